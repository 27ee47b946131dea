// ez_decompress_brk.hip — K2b: the batch Break index (ez_stream_breaks_batch): every stream's Break
// positions without decoding.
//
// Writer.WriteBreak (writer.go:352-366) frames messages inside a stream; Reader.Read returns ErrBreak at
// each marker (reader.go:66-75, :312-313), and the batch decoders skip them.  K2b lists, per stream, the
// output position of every ErrBreak a Reader returns before the stream's first error.  The walk is
// K2z's and K2g's (ez_decompress_size.hip, ez_decompress_segs.hip: one wave per stream, grid-stride,
// super-blocks of 64 chunks staged in LDS, a chunk per lane, settled by kz_walk, ez_k2_walk.h) over the
// steps of ez_k2_brk.h:
//   sum      kb_sum over each lane's true chain up to the chunk's first event (a MetaReset, a form
//            k2_scan hands over): its output bytes, longest distance and Breaks;
//   reduce   an in-order prefix over the lanes for the output bytes and for the Breaks: a lane's output
//            base and Break-count base;
//   events   in lane order, as kg_stream handles them: the state is brought up to the event from the
//            prefix, and every lane runs kb_walk from there to that chunk's exit (one chain, one state:
//            the walk is wave-uniform);
//   fill     (the fill pass) a lane that holds Breaks before its event runs kb_sum once more with its
//            bases and stores each position: one store per Break from the lane that holds it, at
//            brk_pos[brk_idx[s] + the stream's Breaks before it].  Lane order is chain order: no sort.
// A stop (a hand-over form, a segment that fails the window checks, an unsettled super-block, 2 GiB or
// more, a failed end check) sends the whole stream to the exact decoder run dry (ez_decompress.hip,
// its per-stream Break mode), so the results are the exact decoder's by construction.
// The stages, on the caller's stream, with no read-back between them:
//   header       hipMemsetAsync of the workspace's 16 header words (word 15: the hand-over list's length);
//   count        k2b_walk<C, false> over every stream: out_size, status and brk_idx[s] = its Breaks, or
//                brk_idx[s] = 0 and the stream appended to the list; handed[s] says which;
//   exact count  the exact decoder over the list: out_size, status, brk_idx[s];
//   scan         k2b_scan, one block: brk_idx becomes the exclusive scan; brk_total = {written, found},
//                written = found where found <= brk_cap, else 0.  brk_total[0] == 0 is the gate that
//                tells both fill stages there is nothing to do (it is there without a workspace too);
//   fill         k2b_walk<C, true> over the streams that own Breaks and were not handed over;
//   exact fill   the exact decoder over the list once more, for the listed streams that own Breaks.
// Without a workspace the two exact stages run over the whole batch.  A stream without Breaks is
// walked once.
// The parts route (ez_decompress_brk_parts.hip) takes the streams that have parts where
// breaks_parts_route picks it and the caller gave in_bytes: its layout, first and order passes go in
// front of the count stage and its fill pass in front of the fill stage; k2b_walk, with the route's gate
// and part bases in its arguments, then walks only the streams without parts (all of them where the
// gate stayed closed).
#include <hip/hip_runtime.h>

#include "ez_bytes.h"
#include "ez_cache.h"
#include "ez_internal.h"
#include "ez_k2_brk_walk.h"

namespace ez {
namespace {

// One stream b[0 .. nb) by the whole wave.  FILL: put(k, out) is called for Break k of the stream, by
// the lane that holds it (lane 0 for the Breaks behind an event).  Returns the stream's state and where
// its chain ended (both wave-uniform).
struct KbEnd {
    KbState st;
    uint32_t end;
};
template <int C, bool FILL, class Put>
__device__ __forceinline__ KbEnd kb_stream(uint8_t *stage, uint32_t (*bm)[C / 32 + 1], const uint8_t *b, uint32_t nb, int32_t lim32,
                                           int64_t limit, Put put) {
    KbState st = kb_start();
    uint32_t sb = 0;
    while (!st.stop && sb < nb) {
        const uint32_t x = kb_block<C, FILL>(stage, bm, b, nb, sb, sb, sb, lim32, limit, st, put);
        if (st.stop) break;
        sb = x;
    }
    return KbEnd{st, sb};
}

// the count pass (FILL false) and the fill pass over every stream, a wave each, grid-stride
template <int C, bool FILL>
__global__ __launch_bounds__(64) void k2b_walk(BrkArgs A) {
    constexpr int W = C / 32;
    __shared__ __attribute__((aligned(16))) uint8_t stage[kz_stage_bytes(C)];
    __shared__ uint32_t bm[kZLanes][W + 1];  // (+1: the lanes' rows on distinct banks)
    if (FILL && A.brk_total[0] == 0) return;  // (no Break, or more than brk_cap: nothing to write)
    const int lane = lane_id();
    const int64_t limit = A.block_size_limit;
    const int32_t lim32 = k2_lim32(limit);
    const bool parted = A.parts_gate && *A.parts_gate;  // (the parts route walks the streams that have parts)
    for (uint64_t s = blockIdx.x; s < A.count; s += gridDim.x) {
        if (parted && A.parts_base[s] != A.parts_base[s + 1]) continue;
        uint64_t g0 = 0, n = 0;
        if (FILL) {
            g0 = A.brk_idx[s];
            n = A.brk_idx[s + 1] - g0;
            if (n == 0 || A.handed[s]) continue;  // (the exact decoder fills the listed streams)
        }
        const uint64_t nb64 = A.in_off[s + 1] - A.in_off[s];
        bool ok = nb64 < (1ull << 31);
        KbEnd r{kb_start(), 0};
        if (ok) {
            const uint32_t nb = (uint32_t)nb64;
            r = kb_stream<C, FILL>(stage, bm, A.in + A.in_off[s], nb, lim32, limit, [&](uint32_t k, uint64_t out) {
                if (k < n) A.brk_pos[g0 + k] = out;
            });
            ok = kb_end_ok(r.st, r.end, nb);
        }
        if (!FILL && lane == 0) {
            A.handed[s] = ok ? 0u : 1u;
            if (ok) {
                A.out_size[s] = r.st.total;
                if (A.status) A.status[s] = EZ_OK;
                A.brk_idx[s] = r.st.nbrk;
            } else {
                A.brk_idx[s] = 0;
                const uint32_t at = atomicAdd(&A.list[0], 1u);
                A.list[1 + at] = (uint32_t)s;
            }
        }
    }
}

// brk_idx[0 .. count) holds every stream's Breaks: one block turns it into the exclusive scan
// (brk_idx[count] = the Breaks found) and writes brk_total
constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void k2b_scan(BrkArgs A) {
    __shared__ uint64_t part[kScanThreads];
    const uint64_t per = (A.count + kScanThreads - 1) / kScanThreads;
    const uint64_t lo = (uint64_t)threadIdx.x * per < A.count ? (uint64_t)threadIdx.x * per : A.count;
    const uint64_t hi = lo + per < A.count ? lo + per : A.count;
    uint64_t sum = 0;
    for (uint64_t s = lo; s < hi; s++) sum += A.brk_idx[s];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const uint64_t v = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    const uint64_t found = part[kScanThreads - 1];
    uint64_t run = part[threadIdx.x] - sum;
    for (uint64_t s = lo; s < hi; s++) {
        const uint64_t n = A.brk_idx[s];
        A.brk_idx[s] = run;
        run += n;
    }
    if (threadIdx.x == 0) {
        A.brk_idx[A.count] = found;
        A.brk_total[0] = found <= A.brk_cap ? found : 0;
        A.brk_total[1] = found;
    }
}

}  // namespace

// [header: 16 words, word 15 = the hand-over list's length][the list: count words][handed: count words]
uint64_t breaks_workspace_bytes(uint64_t count) { return (64 + count * 8 + 15) & ~(uint64_t)15; }

hipError_t launch_breaks(const BrkArgs &a0, uint64_t max_len, void *workspace, hipStream_t st) {
    BrkArgs a = a0;
    hipError_t e;
    a.parts_gate = a.parts_base = nullptr;
    // The parts route needs the batch's extent to size its records without a read-back (the caller's
    // in_bytes hint) and the workspace's list for the streams it hands over.
    int pchunk = workspace ? breaks_parts_route(max_len, a.count, a.in_bytes) : 0;
    breaks_parts_none();  // (until the route's scratch is leased: the last query did not take it)
    CacheLease please;    // (held until the last launch)
    void *pws = nullptr;
    uint64_t pws_cap = 0;
    if (a.count != 0) {
        const int chunk = size_chunk(max_len);
        // every wave of the chip busy at most (32 per CU); the streams beyond go round the grid
        const unsigned grid = (unsigned)(a.count < 8192 ? a.count : 8192);
        DecompressArgs d{};
        d.in = a.in;
        d.in_off = a.in_off;
        d.out_size = a.out_size;
        d.status = a.status;
        d.count = a.count;
        d.block_size_limit = a.block_size_limit;
        d.dry = 1;
        if (workspace) {
            a.list = (uint32_t *)workspace + 15;
            a.handed = (uint32_t *)workspace + 16 + a.count;
            d.slow = a.list;
            if ((e = hipMemsetAsync(workspace, 0, 64, st)) != hipSuccess) return e;
            if (pchunk) {
                e = launch_breaks_parts(a, pchunk, st, please, &pws, &pws_cap);
                if (e == hipErrorOutOfMemory) {  // (no scratch: the wave route)
                    pchunk = 0;
                    a.parts_gate = a.parts_base = nullptr;
                } else if (e != hipSuccess) {
                    return e;
                }
            }
            if (chunk == 64) hipLaunchKernelGGL((k2b_walk<64, false>), dim3(grid), dim3(64), 0, st, a);
            else if (chunk == 1024) hipLaunchKernelGGL((k2b_walk<1024, false>), dim3(grid), dim3(64), 0, st, a);
            else hipLaunchKernelGGL((k2b_walk<256, false>), dim3(grid), dim3(64), 0, st, a);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        d.brk_n = a.brk_idx;
        if ((e = launch_exact_dry(d, st)) != hipSuccess) return e;
        hipLaunchKernelGGL(k2b_scan, dim3(1), dim3(kScanThreads), 0, st, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (workspace) {
            if (pchunk && (e = launch_breaks_parts_fill(a, pchunk, pws, pws_cap, st)) != hipSuccess) return e;
            if (chunk == 64) hipLaunchKernelGGL((k2b_walk<64, true>), dim3(grid), dim3(64), 0, st, a);
            else if (chunk == 1024) hipLaunchKernelGGL((k2b_walk<1024, true>), dim3(grid), dim3(64), 0, st, a);
            else hipLaunchKernelGGL((k2b_walk<256, true>), dim3(grid), dim3(64), 0, st, a);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        d.brk_n = nullptr;
        d.brk_base = a.brk_idx;
        d.brk_out = a.brk_pos;
        d.brk_gate = a.brk_total;
        return launch_exact_dry(d, st);
    }
    hipLaunchKernelGGL(k2b_scan, dim3(1), dim3(kScanThreads), 0, st, a);  // (brk_idx[0] = 0, brk_total = {0, 0})
    return hipGetLastError();
}

}  // namespace ez
