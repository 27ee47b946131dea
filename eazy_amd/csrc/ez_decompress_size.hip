// ez_decompress_size.hip — K2z: each stream's decoded length without decoding (ez_decompressed_size_batch).
//
// A decoded length depends on the tokens alone (Reader.read reader.go:143-216 adds every token's
// length, whatever its bytes are), so the query reads token headers, skips every literal's body and
// writes one u64 per stream.  One wave per stream, grid-stride over the streams.  The token chain is
// cut inside the wave by speculation: the stream is taken in super-blocks of 64 chunks of C input
// bytes, a chunk per lane.  Per super-block, which starts at the true chain's position sb:
//   walk     kz_walk (ez_k2_walk.h): the super-block's 64 x C bytes and the 16 a header at its end reads
//            are staged in LDS, and the wave settles every lane's entry and exit on the true chain (a
//            super-block that does not settle within the bound hands the stream over);
//   sum      kz_sum (ez_k2_size.h) over each lane's true chain;
//   reduce   an in-order prefix over the lanes for the output bytes and the reset-before-any-output
//            rule; the totals, the window and the flags are carried.
// The next super-block starts at lane 63's true exit: a literal's body is never staged or read, however
// long it is.  At the stream's end kz_end_ok decides: the wave writes out_size[s] and EZ_OK, or appends
// the stream to the slow list -- every error, every form k2_scan hands over, a MetaReset after output, a
// stream of 2 GiB or more.  Nothing else is written.  The list goes to K2g's stage (k2g_size,
// ez_decompress_segs.hip), which sizes the streams with MetaResets after output, and what that hands on
// to the exact decoder run dry (ez_decompress.hip).
#include <hip/hip_runtime.h>

#include "ez_bytes.h"
#include "ez_internal.h"
#include "ez_k2_walk.h"

namespace ez {
namespace {

template <int C>
__global__ __launch_bounds__(64) void k2z_size(DecompressArgs A) {
    constexpr int W = C / 32;
    __shared__ __attribute__((aligned(16))) uint8_t stage[kz_stage_bytes(C)];
    __shared__ uint32_t bm[kZLanes][W + 1];  // (+1: the lanes' rows on distinct banks)
    const bool parted = A.size_gate && *A.size_gate;  // (the parts route sized the streams that have parts)
    const int lane = lane_id();
    const int64_t limit = A.block_size_limit;
    const int32_t lim32 = k2_lim32(limit);
    for (uint64_t s = blockIdx.x; s < A.count; s += gridDim.x) {
        if (parted && A.size_base[s] != A.size_base[s + 1]) continue;
        const uint64_t nb64 = A.in_off[s + 1] - A.in_off[s];
        const uint8_t *b = A.in + A.in_off[s];
        bool bad = nb64 >= (1ull << 31);
        const uint32_t nb = bad ? 0u : (uint32_t)nb64;
        uint32_t sb = 0, maxd = 0;
        uint64_t total = 0;
        int32_t bsl = -1;
        while (!bad && sb < nb) {
            const KzWalk k = kz_walk<C>(stage, bm, b, nb, sb, sb, true, sb);
            if (!k.settled) {
                bad = true;
                break;
            }
            const KzSum r = kz_sum<C>(KzWin{stage, sb}, sb, lane, nb, k.a, k.x, lim32, limit);
            const uint64_t io = wscan_add_u64(r.out);
            maxd = max(maxd, wmax_u32(r.maxd));
            if (wballot((r.fl & kZBad) || kz_reset_bad(r.fl, total + io - r.out))) bad = true;
            const uint64_t rm = wballot((r.fl & kZReset) != 0);
            if (rm) bsl = (int32_t)((__shfl((int)r.fl, 63 - __builtin_clzll(rm), kWave) >> 8) & 0xff);
            total += __shfl(io, kWave - 1, kWave);
            sb = __shfl(k.x, kWave - 1, kWave);
        }
        if (!bad) bad = !kz_end_ok(sb, nb, total, bsl, maxd);
        if (lane == 0) {
            if (bad) {
                slow_append(A, s);
            } else {
                A.out_size[s] = total;
                if (A.status) A.status[s] = EZ_OK;
            }
        }
    }
}

// A lane per stream, for large batches of short streams: each lane walks its stream's whole chain in
// order (kz_serial), reading 16 bytes per token through the caches.  No speculation, so nothing is
// walked twice, and 64 streams share a wave's instructions: with enough short streams to fill the
// chip's lanes that beats a wave per stream, whose lanes mostly repeat each other's walks on a stream
// of a few dozen chunks (C1: DESIGN §4 K2z).
__global__ __launch_bounds__(64) void k2z_lane(DecompressArgs A) {
    const bool parted = A.size_gate && *A.size_gate;  // (the parts route sized the streams that have parts)
    const int64_t limit = A.block_size_limit;
    const int32_t lim32 = k2_lim32(limit);
    for (uint64_t s = (uint64_t)blockIdx.x * kWave + threadIdx.x; s < A.count; s += (uint64_t)gridDim.x * kWave) {
        if (parted && A.size_base[s] != A.size_base[s + 1]) continue;
        const uint64_t nb64 = A.in_off[s + 1] - A.in_off[s];
        const uint8_t *b = A.in + A.in_off[s];
        uint64_t total = 0;
        bool ok = nb64 < (1ull << 31);
        if (ok) {
            const uint32_t nb = (uint32_t)nb64;
            ok = kz_serial(kz_global_at(b, nb), nb, lim32, limit, total);
        }
        if (ok) {
            A.out_size[s] = total;
            if (A.status) A.status[s] = EZ_OK;
        } else {
            slow_append(A, s);
        }
    }
}

}  // namespace

// The chunk size for the caller's hint (the longest input stream, 0 = unknown): 64 bytes up to 4 KiB,
// so that a C1-sized stream's ~2 KiB of input spans half a wave; 256 bytes up to 512 KiB; 1 KiB
// above, for the few long streams of a bucket batch (fewer super-blocks, and a warm-up long enough
// that almost every lane's speculation has met the true chain).  (Measured: DESIGN §4 K2z.)
int size_chunk(uint64_t max_len) { return max_len == 0 ? 256 : (max_len <= 4096 ? 64 : (max_len <= (512u << 10) ? 256 : 1024)); }

// Batches of at least this many streams whose hint says they are short take the lane-per-stream
// kernel: from here on its one walk per stream, 64 streams to a wave, costs less than the wave
// kernel's several walks per stream (an estimate from the wave kernel's C1 time per stream and the
// length of one serial walk, not a measured crossover; below it the wave kernel's parallelism inside
// a stream is what a few streams need).  Reported as chunk 1.
constexpr uint64_t kZLaneStreams = 4096;
int size_route(uint64_t max_len, uint64_t count) {
    return max_len != 0 && max_len <= 4096 && count >= kZLaneStreams ? 1 : size_chunk(max_len);
}

// The parts route's chunk for a batch, 0: the wave route, which takes every batch whose caller did not
// give its input bytes, an empty one, one of more than 2^20 streams, and all of them under
// ez_select_size_route('v').  Forced (ez_select_size_route('p')): at any length, 1,024 where the wave
// route takes 1,024, else 256.
// Automatic, only where it measured faster than a wave per stream (tools/size_parts_bench.py, DESIGN
// §4 K2z; ms, wave / parts 256 / parts 1,024):
//   one stream from 240 KiB of input on, chunk 1,024 (one log stream of 0.25 MB compressed 1.76 / 0.70 /
//     0.38, 0.5 MB 3.51 / 0.99 / 0.39, 2 MB 9.61 / 3.19 / 0.40, 8 MB 38.7 / 15.4 / 0.77, 32 MB 157 / 62.6 /
//     1.81: chunk 256 leaves a quarter of the parts to the one wave that walks them again);
//   2 to 64 streams whose longest is over 512 KiB, chunk 256 (C4s, 64 x 0.9 MB: 7.23 / 1.37 / 2.21; C4's
//     literals are the wave route's by the probe: 0.073 on the wave route alone, 0.052 automatic).
// More streams keep a wave each, which fills the chip (1,024 x 1 MiB logs 4.06 / 4.48 / 6.64, C2 2.25 /
// 3.58 / 6.25).
int size_parts_route(uint64_t max_len, uint64_t count, uint64_t in_bytes) {
    const int sel = selected_size_route();
    if (count == 0 || in_bytes == 0 || count > (1u << 20) || sel == 'v') return 0;
    if (sel == 'p') return size_chunk(max_len) == 1024 ? 1024 : 256;
    if (count == 1) return max_len >= (240u << 10) ? 1024 : 0;
    return count <= 64 && max_len > (512u << 10) ? 256 : 0;
}

hipError_t launch_size_fast(const DecompressArgs &a, int chunk, hipStream_t st) {
    if (chunk == 1) {
        const uint64_t blocks = (a.count + kWave - 1) / kWave;
        hipLaunchKernelGGL(k2z_lane, dim3((unsigned)(blocks < (1u << 20) ? blocks : (1u << 20))), dim3(64), 0, st, a);
        return hipGetLastError();
    }
    // every wave of the chip busy at most (32 per CU); the streams beyond go round the grid
    const unsigned grid = (unsigned)(a.count < 8192 ? a.count : 8192);
    if (chunk == 64) hipLaunchKernelGGL(k2z_size<64>, dim3(grid), dim3(64), 0, st, a);
    else if (chunk == 1024) hipLaunchKernelGGL(k2z_size<1024>, dim3(grid), dim3(64), 0, st, a);
    else hipLaunchKernelGGL(k2z_size<256>, dim3(grid), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace ez
