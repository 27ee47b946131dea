// ez_k1_long.hip — K1L's kernels and launchers: k1_long (long fresh streams of a batch, and the
// streams K1x or K1c hand over), k1_long_ring / k1_ring_store (one Write on a Writer handle) and
// k1_long_rings (one Write on each of many handles).
// The parse loop itself is ez_k1_long.h's long_loop.
#include "ez_k1_long.h"
#include "ez_k1_emit.h"
#include "ez_k1_internal.h"

namespace ez {
namespace k1 {  // (beside long_loop's other sources: WindowFromSrc is specialised for LdsSrc)

// a Writer handle's Write as long_loop's source (see FreshSrc)
struct RingSrc {
    const uint8_t *p, *blo, *bhi;  // the Write (blo = p, bhi = p + n)
    const uint8_t *ring;
    int64_t start;
    uint32_t mask;
    __device__ __forceinline__ V16 ring_at(int32_t y) const {  // 16 ring bytes of positions y .. y+15 (< 0)
        const uint32_t r = (uint32_t)((start + y) & mask);
        if (r + 16 <= mask + 1) return ld16v(ring + r);
        V16 v{0, 0};
        for (int t = 0; t < 16; t++) {
            const uint64_t c = ring[(r + t) & mask];
            if (t < 8) v.lo |= c << (8 * t);
            else v.hi |= c << (8 * (t - 8));
        }
        return v;
    }
    __device__ __forceinline__ void around(int32_t y, uint64_t &before, uint64_t &from) const {
        V16 v;
        if (y - 8 >= 0) {
            const uint8_t *a = p + (y - 8);
            v = a + 16 <= bhi ? ld16v(a) : ld_clamped(a, blo, bhi);  // (past the Write: 0)
        } else if (y + 8 <= 0) {
            v = ring_at(y - 8);
        } else {  // across the Write's start: the ring's bytes, then p's
            const V16 r = ring_at(y - 8);
            const uint8_t *a = p;
            const V16 q = a + 16 <= bhi ? ld16v(a) : ld_clamped(a, blo, bhi);
            const uint32_t k = (uint32_t)(8 - y);  // ring bytes (1 .. 15)
            const V16 qs = shl16(q, k), m = keep_low16(V16{~0ull, ~0ull}, (int32_t)k);
            v = V16{(r.lo & m.lo) | (qs.lo & ~m.lo), (r.hi & m.hi) | (qs.hi & ~m.hi)};
        }
        before = v.lo;
        from = v.hi;
    }
    __device__ __forceinline__ void bytes48(int32_t cand, V16 &c0, V16 &c1, V16 &c2) const {
        around(cand, c0.lo, c0.hi);
        around(cand + 16, c1.lo, c1.hi);
        around(cand + 32, c2.lo, c2.hi);
    }
};

// LdsSrc: RingSrc with the Write and the ring's last bytes before it staged in LDS (a handle's Write of
// at most kLdsWrite bytes): lds + kLdsRing + y holds position y for -rl <= y < n + 64 (zeros past
// the Write); the window's bytes and the candidates' come from there, anything else from RingSrc.
constexpr int32_t kLdsRing = 32768, kLdsWrite = 49152;
static_assert(kLdsWrite == (int32_t)kHandleLdsWrite, "the handle path's zero-copy bound is K1L's LDS-staged Write");
struct LdsSrc {
    const uint8_t *lds;
    int32_t rl, n;
    RingSrc g;  // (the window's bytes come from here too: WindowFromSrc)
    __device__ __forceinline__ void around(int32_t y, uint64_t &before, uint64_t &from) const {
        if (y - 8 >= -rl && y + 8 <= n + 64) {
            const uint8_t *q = lds + kLdsRing + (y - 8);
            before = *(const u64_ua *)q;
            from = *(const u64_ua *)(q + 8);
        } else {
            g.around(y, before, from);
        }
    }
    __device__ __forceinline__ static V16 lds16(const uint8_t *q) { return V16{*(const u64_ua *)q, *(const u64_ua *)(q + 8)}; }
    __device__ __forceinline__ void bytes48(int32_t cand, V16 &c0, V16 &c1, V16 &c2) const {
        if (cand - 8 >= -rl && cand + 40 <= n + 64) {  // one check for the 48 bytes
            const uint8_t *q = lds + kLdsRing + (cand - 8);
            c0 = lds16(q);
            c1 = lds16(q + 16);
            c2 = lds16(q + 32);
        } else {
            g.around(cand, c0.lo, c0.hi);
            g.around(cand + 16, c1.lo, c1.hi);
            g.around(cand + 32, c2.lo, c2.hi);
        }
    }
    // the window's bytes x-8 .. x+39 (0 <= x < n: always staged)
    __device__ __forceinline__ void window48(int32_t x, V16 &w0, V16 &w1, V16 &w2) const {
        const uint8_t *q = lds + kLdsRing + (x - 8);
        w0 = lds16(q);
        w1 = lds16(q + 16);
        w2 = lds16(q + 32);
    }
};
template <>
struct WindowFromSrc<LdsSrc> {
    static constexpr bool value = true;
};

}  // namespace k1
namespace {
using namespace k1;

// a group of 16 lanes per stream, 4 streams per wave; spec_mode 2: K1x's streams resume
// spw: streams per wave (1, 2 or 4; the other lane groups idle, with no table): a batch of few long
// streams runs more waves per SIMD, each a lone latency chain, instead of fewer waves of 4 streams
// only (K1c's fallback): the streams whose only[ostride s] is nonzero, the others untouched (nullptr: all)
__global__ __launch_bounds__(64) void k1_long(CompressArgs A, uint32_t table_words, uint4 *recs, uint64_t rcap, uint32_t spw,
                                              const uint32_t *only, uint32_t ostride) {
    constexpr int G = 16;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = (int)(threadIdx.x & 63);
    const int g = lane / G, lj = lane % G;
    const bool grp = (uint32_t)g < spw;
    const uint32_t hsh = 32u - (uint32_t)(64 - __builtin_clzll((uint64_t)(A.hs - 1)));
    uint32_t *htw = (uint32_t *)smem + (uint32_t)(grp ? g : 0) * table_words;  // (an idle group never touches it)
    const uint64_t s = (uint64_t)blockIdx.x * spw + (uint32_t)g;
    const bool spec = A.spec_mode != 0;
    bool have = grp && s < A.count;
    if (have && spec && A.spec[s].flags != 0) have = false;  // finished by K1x
    if (have && only && only[(uint64_t)ostride * s] == 0) have = false;  // K1c took it
    const uint8_t *blo = A.in, *bhi = A.in + A.in_off[A.count];
    int32_t n = 0, i = 0, done = 0;
    const uint8_t *p = blo;
    if (have) {
        n = (int32_t)(A.in_off[s + 1] - A.in_off[s]);
        p = A.in + A.in_off[s];
        if (spec) {
            i = (int32_t)A.spec[s].from;
            done = (int32_t)A.spec[s].done;
        }
    }
    if (grp)
        for (int32_t k = lj; k < (int32_t)A.hs; k += G) htw[k] = have && spec ? A.spec_tab[s * (uint64_t)A.hs + k] : 0u;
    int err = have && (uint64_t)n > A.max_len ? EZ_EINVAL : (have ? 0 : EZ_EINVAL);
    int32_t nrec = 0;
    // (the groups' window buffers after the tables)
    uint8_t *wl = smem + (size_t)spw * table_words * 4 + (size_t)g * kWinLdsBytes;  // (idle groups too: their own buffers)
    long_loop<FreshSrc, true>(FreshSrc{{p, blo, bhi}}, p, n, i, done, A.bs, lj, g, htw, hsh, recs + (have ? s * rcap : 0), rcap, blo, bhi,
                              nrec, err, wl);
    if (have && lj == 0) A.out_size[s] = (uint64_t)nrec | ((uint64_t)err << 48);
}

// K1L on a Writer handle (Writer.Write writer.go:206-337 on a stream at position start): one 16-lane
// group, the handle's table (uint32 stream positions) in LDS as positions relative to the Write (far
// ones clamped: the far skip, writer.go:219-221, still sees them as far), the history before the Write
// from the handle's ring (RingSrc).  The table goes back to the handle, converted back, at the end.
constexpr int32_t kRelFar = 1 << 28;  // |relative position| clamp (bs <= 2^26, Writes < 2^27 bytes)

// the staged ring bytes for a Write of n bytes: 16 n, at least kRingMin, at most kLdsRing
#ifndef EZ_K1R_RL
#define EZ_K1R_RL 32768
#endif
__device__ __forceinline__ int32_t knob_dev_rl(int32_t n) {
    const int32_t r = 16 * n < EZ_K1R_RL ? EZ_K1R_RL : (16 * n > kLdsRing ? kLdsRing : ((16 * n + 15) & ~15));
    return r > kLdsRing ? kLdsRing : r;
}
// one Write on one handle by one 256-thread block: k1_long_ring's whole work (A: the handle's args,
// count 1; recs: the block's rcap records)
template <bool LDS>
__device__ __forceinline__ void long_ring_block(const CompressArgs &A, uint4 *recs, uint64_t rcap) {
    constexpr int G = 16;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = (int)threadIdx.x, lane = tid & 63;  // 4 waves stage; wave 0's first group parses
    const int g = lane / G + 4 * (tid >> 6), lj = lane % G;
    const uint32_t hsh = 32u - (uint32_t)(64 - __builtin_clzll((uint64_t)(A.hs - 1)));
    uint32_t *htw = (uint32_t *)smem;
    const uint8_t *p = A.in + A.in_off[0];
    const int32_t n = (int32_t)(A.in_off[1] - A.in_off[0]);
    uint8_t *lds = smem + (size_t)A.hs * 4;
    // the ring's last rl bytes staged before the Write (older candidates read the ring in HBM; staging
    // less for small Writes measured no faster: 100-byte Writes 26.2 / 27.2 against 26.8 / 25.2 us at
    // 4 KiB and 32 KiB, two alternating runs; -DEZ_K1R_RL=<bytes> builds for A/B)
    static_assert(kLdsRing % 16 == 0, "");
    const int32_t want = knob_dev_rl(n);
    const int32_t rl = A.bs < want ? (int32_t)A.bs : want;
    const uint32_t mask = (uint32_t)(A.bs - 1);
    if (LDS) {  // the ring's last rl bytes, the Write, 64 zeros: 16 bytes per lane and step, 4 loads in flight
        const RingSrc R{p, p, p + n, A.ring, A.start, mask};
        for (int32_t y0 = -rl + 16 * tid; y0 < n + 64; y0 += 4 * 16 * 256) {
            V16 v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int32_t y = y0 + u * 16 * 256;
                if (y < 0) v[u] = R.ring_at(y);  // (rl is a multiple of 16: no piece straddles the Write's start)
                else v[u] = p + y + 16 <= p + n ? ld16v(p + y) : (y < n ? ld_clamped(p + y, p, p + n) : V16{0, 0});
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int32_t y = y0 + u * 16 * 256;
                if (y < n + 64) {
                    *(u64_ua *)(lds + kLdsRing + y) = v[u].lo;
                    *(u64_ua *)(lds + kLdsRing + y + 8) = v[u].hi;
                }
            }
        }
    }
    // the table by the whole block (the parse below is one group's)
#pragma unroll 4
    for (int32_t k = tid; k < (int32_t)A.hs; k += 256) {
        int64_t r = (int64_t)A.ht_global[k] - A.start;
        r = r < -kRelFar ? -kRelFar : (r > kRelFar ? kRelFar : r);
        htw[k] = (uint32_t)(int32_t)r;
    }
    __syncthreads();
    int err = 0;
    int32_t nrec = 0;
    if (g == 0) {  // one group (the other lanes idle)
        const RingSrc P{p, p, p + n, A.ring, A.start, mask};
        if (LDS) long_loop(LdsSrc{lds, rl, n, P}, p, n, 0, 0, A.bs, lj, 0, htw, hsh, recs, rcap, p, p + n, nrec, err);
        else long_loop(P, p, n, 0, 0, A.bs, lj, 0, htw, hsh, recs, rcap, p, p + n, nrec, err);
    }
    __syncthreads();
    for (int32_t k = tid; k < (int32_t)A.hs; k += 256) {
        const int32_t r = (int32_t)htw[k];
        if (r != -kRelFar && r != kRelFar) A.ht_global[k] = (uint32_t)(A.start + r);
    }
    if (LDS) {  // the Write into the handle's ring (k1_ring_store's work; the parse has read the ring)
        const int32_t from = (int64_t)n > A.bs ? (int32_t)(n - A.bs) : 0;
        for (int32_t k = from + 16 * tid; k < n; k += 16 * 256) {
            const uint32_t r = (uint32_t)((A.start + k) & mask);
            const uint8_t *q = lds + kLdsRing + k;
            if (k + 16 <= n && r + 16 <= mask + 1) {
                *(u64_ua *)(A.ring + r) = *(const u64_ua *)q;
                *(u64_ua *)(A.ring + r + 8) = *(const u64_ua *)(q + 8);
            } else {
                for (int32_t t = 0; t < 16 && k + t < n; t++) A.ring[(r + (uint32_t)t) & mask] = q[t];
            }
        }
    }
    if (tid == 0) A.out_size[0] = (uint64_t)nrec | ((uint64_t)err << 48);
    if (LDS) {
        // the token writer (k1_emit's emit_stream) by wave 0 of the same block: one launch per Write
        __threadfence();
        __syncthreads();
        if (tid < 64) emit_stream<true>(A, (const uint64_t *)recs, rcap, 0, lane);
        if (A.done_flag) {
            __syncthreads();
            if (tid == 0) {
                __threadfence_system();
                __hip_atomic_store(A.done_flag, A.done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

template <bool LDS>
__global__ __launch_bounds__(256) void k1_long_ring(CompressArgs A, uint4 *recs, uint64_t rcap) {
    long_ring_block<LDS>(A, recs, rcap);
}

// One Write on each of gridDim.x handles (ez_writer_write_many): block b is k1_long_ring<true> for
// handle b, whose ring, table and sizes it reads from desc[b] and whose in_off[2] out_off[2] out_size
// status words are meta[6 b ..]; offsets count from D, the call's staging buffer.  The blocks share
// nothing: each has its own handle (the host refuses a handle named twice), meta words, output slot
// and rcap records.  The LDS layout is the one-handle kernel's with this block's own table size.
__global__ __launch_bounds__(256) void k1_long_rings(uint8_t *D, uint64_t *meta, const RingDesc *desc, uint4 *recs, uint64_t rcap) {
    const RingDesc d = desc[blockIdx.x];
    uint64_t *m = meta + 6 * (uint64_t)blockIdx.x;
    CompressArgs A{};
    A.in = D;
    A.in_off = m;
    A.out = D;
    A.out_off = m + 2;
    A.out_size = m + 4;
    A.status = (int32_t *)(m + 5);
    A.count = 1;
    A.bs = d.bs;
    A.hs = d.hs;
    A.append_magic = d.append_magic;
    A.ver = 0;
    A.header = d.header;
    A.start = d.start;
    A.ring = d.ring;
    A.ht_global = d.ht;
    A.max_len = m[1] - m[0];
    long_ring_block<true>(A, recs + (uint64_t)blockIdx.x * rcap, rcap);
}

// the Write's last min(n, bs) bytes into the handle's ring (block[(start + k) & mask], copyData)
__global__ __launch_bounds__(256) void k1_ring_store(CompressArgs A) {
    const uint8_t *p = A.in + A.in_off[0];
    const int64_t n = (int64_t)(A.in_off[1] - A.in_off[0]);
    const int64_t from = n > A.bs ? n - A.bs : 0;
    const uint64_t mask = (uint64_t)A.bs - 1;
    for (int64_t k = from + (int64_t)(blockIdx.x * 256 + threadIdx.x); k < n; k += (int64_t)gridDim.x * 256)
        A.ring[(uint64_t)(A.start + k) & mask] = p[k];
}

}  // namespace

// K1L: long fresh single-Write streams (table <= 4096 entries, positions < 2^31, LDS lane order);
// EZ_K1L=0 turns it off (A/B: K1x's continuation on the general kernel)
bool long_applies(const CompressArgs &a) {
    static const bool off = knob("EZ_K1L", 1) == 0;
    return !off && !a.ring && !a.write_idx && a.start == 0 && a.header && a.hs <= 4096 && a.hs >= 4 && a.max_len > 0 &&
           a.max_len < (1ull << 31) && lds_store32_in_lane_order();
}

// [K1L's records][the token writer's workspace][K1c's workspace]
uint64_t long_scratch_bytes(const CompressArgs &a) {
    const uint64_t r = up256(a.count * rec_cap(a) * sizeof(WideRec)) + ew_bytes(a);
    return chunk_applies(a) ? r + chunk_scratch_bytes(a) : r;
}

// k1_long, S streams per wave: the S tables, then the window regions of the wave's four groups in
// LDS (WinLdsL; C2 K1 25.8 -> 24.9 ms, C4s 254 -> 246 against the region in registers).  launch_long
// runs it on every stream; K1c (launch_chunk) on the streams it could not prove, marked by `only`
hipError_t launch_k1_long(const CompressArgs &a, uint4 *recs, uint64_t rcap, uint32_t S, const uint32_t *only, uint32_t ostride,
                          hipStream_t st) {
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void *)k1_long, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_done = true;
    }
    const size_t lds = (size_t)S * (size_t)a.hs * 4 + (size_t)4 * kWinLdsBytes;
    const unsigned grid = (unsigned)((a.count + S - 1) / S);
    hipLaunchKernelGGL(k1_long, dim3(grid), dim3(64), lds, st, a, (uint32_t)a.hs, recs, rcap, S, only, ostride);
    return hipGetLastError();
}

hipError_t launch_long(const CompressArgs &a, uint8_t *recs, hipStream_t st) {
    if (chunk_applies(a)) return launch_chunk(a, recs, st);
    // streams per wave: one for batches of a few hundred streams (C4s' 64: K1 361 -> 291 ms), else 4
    // (each wave's instructions serve 4 streams; C2's 4,096 streams: 32.3 ms at 4, 33.5 at 2, 38.2 at
    // 1; 1,024 x 1 MiB compressed at 7.3 GiB/s at 1 against 7.6 at 4); EZ_K1L_SPW=1|2|4 overrides
    static const uint32_t spw_env = (uint32_t)knob("EZ_K1L_SPW", 0);
    const uint32_t S = spw_env == 1 || spw_env == 2 || spw_env == 4 ? spw_env : (a.count <= 256 ? 1u : 4u);
    const uint64_t rcap = rec_cap(a);
    const hipError_t e = launch_k1_long(a, (uint4 *)recs, rcap, S, nullptr, 0u, st);
    if (e != hipSuccess) return e;
    set_compress_route("l");
    return launch_emit_wide(a, (const uint4 *)recs, rcap, recs + up256(a.count * rcap * sizeof(WideRec)), st);
}

// K1L for one Write on a Writer handle (writer_run): single Writes of 16 bytes .. 64 MiB on
// handles with version 0, a table of at most 4096 entries, bs <= 2^26, positions below 2^32
// (the uint32 table values stay exact: a Write across 2^32 takes the general kernel)
bool long_ring_applies(const CompressArgs &a) {
    return a.count == 1 && a.ring && !a.write_idx && a.ver == 0 && a.hs <= 4096 && a.hs >= 4 && a.bs <= (1ll << 26) &&
           a.max_len >= 16 && a.max_len < (1ull << 26) && a.start >= 0 && (uint64_t)a.start + a.max_len <= (1ull << 32) &&
           lds_store32_in_lane_order();
}
uint64_t long_ring_scratch_bytes(const CompressArgs &a) { return rec_cap(a) * sizeof(WideRec); }
hipError_t launch_long_ring(const CompressArgs &a, uint8_t *recs, hipStream_t st) {
    const uint64_t rcap = rec_cap(a);
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void *)k1_long_ring<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_done = true;
    }
    // Writes of up to kLdsWrite bytes: the Write and the ring's last bytes in LDS, the token writer in
    // the same kernel
    if (a.max_len <= (uint64_t)kLdsWrite) {
        set_compress_route("hl:lds");
        hipLaunchKernelGGL(k1_long_ring<true>, dim3(1), dim3(256), (size_t)a.hs * 4 + kLdsRing + kLdsWrite + 64, st, a, (uint4 *)recs,
                           rcap);
        return hipGetLastError();
    }
    set_compress_route("hl:global");
    hipLaunchKernelGGL(k1_long_ring<false>, dim3(1), dim3(256), (size_t)a.hs * 4, st, a, (uint4 *)recs, rcap);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = launch_emit(a, (const uint64_t *)recs, rcap, true, st)) != hipSuccess) return e;
    const uint64_t n = a.max_len;
    const uint64_t blocks = (n < (uint64_t)a.bs ? n : (uint64_t)a.bs) / 256 / 16 + 1;
    hipLaunchKernelGGL(k1_ring_store, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, st, a);
    return hipGetLastError();
}

// K1L for one Write on each of `count` handles in one launch (ez_writer_write_many): Writes of 16 ..
// kLdsWrite bytes that long_ring_applies holds for, the longest of `longest` bytes, on tables of at
// most max_hs entries.  D, meta and desc as k1_long_rings reads them; recs: long_rings_scratch_bytes
uint64_t long_rings_rcap(uint64_t longest) { return longest / 6 + 1; }
uint64_t long_rings_scratch_bytes(uint64_t count, uint64_t longest) { return count * long_rings_rcap(longest) * sizeof(WideRec); }
hipError_t launch_long_rings(uint8_t *D, uint64_t *meta, const RingDesc *desc, uint64_t count, int64_t max_hs, uint64_t longest,
                             uint8_t *recs, hipStream_t st) {
    if (count == 0 || count > 0x7fffffffull || longest > (uint64_t)kLdsWrite || max_hs > 4096) return hipErrorInvalidValue;
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void *)k1_long_rings, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_done = true;
    }
    // (the staging loop stores whole 16-byte pieces: the Write's length rounded up)
    const size_t lds = (size_t)max_hs * 4 + kLdsRing + (((size_t)longest + 15) & ~(size_t)15) + 64;
    hipLaunchKernelGGL(k1_long_rings, dim3((unsigned)count), dim3(256), lds, st, D, meta, desc, (uint4 *)recs, long_rings_rcap(longest));
    return hipGetLastError();
}

}  // namespace ez
