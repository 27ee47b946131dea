// ez_k1_emit.hip — K1e, the token writers: k1_emit (a wave per stream, ez_k1_emit.h's
// emit_stream) and, for 16-byte records across the chip, ke_size / ke_scan / ke_write; the host
// entry points the parse families call after their parse.
#include "ez_k1_emit.h"
#include "ez_k1_internal.h"

namespace ez {
namespace {
using namespace k1;

template <bool WIDE>
__global__ __launch_bounds__(256, 8) void k1_emit(CompressArgs A, const uint64_t *recs, uint64_t rcap) {
    __shared__ uint64_t stage[WIDE ? 1 : 4][WIDE ? 1 : kEmitStage];
    __shared__ __attribute__((aligned(16))) uint8_t sin[WIDE ? 1 : 4][WIDE ? 16 : kEmitIn + 32];
    const int lane = (int)(threadIdx.x & 63);
    // the wave's stream, wave-uniform (readfirstlane: its per-stream values live in SGPRs)
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t s = (uint64_t)blockIdx.x * 4 + (uint32_t)w;
    if (s >= A.count) return;
    emit_stream<WIDE>(A, recs, rcap, s, lane, WIDE ? nullptr : &stage[WIDE ? 0 : w][0], WIDE ? nullptr : &sin[WIDE ? 0 : w][0]);
}

// The token writer for 16-byte records (K1L, K1c) across the chip: k1_emit<true> walks a stream's
// records with one wave, 64 at a time (C4s: 64 waves over ~180 k records each, 6.6 ms).  Here blocks
// of kEwRec records each sum their tokens' sizes (ke_size), one wave per stream scans the block sums
// after the header (ke_scan, which also decides the stream's size and status as emit_stream does),
// and every block writes its tokens at their offsets (ke_write).  Tokens, literal bytes and the
// trailing literal are emit_stream's; a token is written when it ends within the slot, and a slot
// too small ends the output at the first token that does not fit (ENOSPC), as emit_stream's does.
constexpr int32_t kEwRec = 2048, kEwPer = kEwRec / 256;
struct EwBufs {
    uint64_t *bsum;   // per (stream, block): the block's token bytes, then (ke_scan) its offset
    uint64_t *info;   // per stream: {records, tail literal start, out end of the records, flags}
    uint32_t nb;      // blocks per stream
};
// the size of record r's tokens (literal tag + bytes, copy tag + offset) and its literal (start, length)
__device__ __forceinline__ int32_t ew_token(const uint4 *rec, int32_t r, int32_t done0, int32_t &lit_at, int32_t &L) {
    const uint4 v = rec[r];
    const int32_t dk = r == 0 ? done0 : (int32_t)(rec[r - 1].x + rec[r - 1].y);
    L = (int32_t)v.x - dk;
    lit_at = dk;
    const bool lit = (v.w & 1) != 0 || L > 0;
    int32_t ln = 0, tn = 0, on = 0;
    (void)tag_bytes(0x00, L, &ln);
    (void)tag_bytes(0x80, (int32_t)v.y, &tn);
    (void)off_bytes((int32_t)v.z, (int32_t)v.y, &on);
    if (v.y == 0) tn = on = 0;
    return (lit ? ln + L : 0) + tn + on;
}
__device__ __forceinline__ void ew_stream(const CompressArgs &A, uint64_t s, int32_t &H, int32_t &done0, bool &skip) {
    const bool spec = A.spec_mode != 0;
    skip = spec && A.spec[s].flags != 0;
    H = spec ? (int32_t)A.spec[s].op : (A.header ? (A.append_magic ? 9 : 3) : 0);
    done0 = spec ? (int32_t)A.spec[s].done : 0;
}

__global__ __launch_bounds__(256) void ke_size(CompressArgs A, const uint4 *recs, uint64_t rcap, EwBufs E) {
    __shared__ uint64_t part[4];
    const uint64_t s = blockIdx.x / E.nb;
    const uint32_t b = blockIdx.x % E.nb;
    int32_t H, done0;
    bool skip;
    ew_stream(A, s, H, done0, skip);
    const int32_t m = (int32_t)((A.out_size[s] & 0xffffffffffffull) < rcap ? (A.out_size[s] & 0xffffffffffffull) : rcap);
    if (skip || (int64_t)b * kEwRec >= m) return;
    const uint4 *rec = recs + s * rcap;
    uint64_t sum = 0;
    for (int32_t t = 0; t < kEwPer; t++) {
        const int32_t r = (int32_t)b * kEwRec + t * 256 + (int32_t)threadIdx.x;
        int32_t la, L;
        if (r < m) sum += (uint64_t)ew_token(rec, r, done0, la, L);
    }
    for (int d = 32; d >= 1; d >>= 1) sum += (uint64_t)__shfl_xor((long long)sum, d, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) E.bsum[s * E.nb + b] = part[0] + part[1] + part[2] + part[3];
}

// a wave per stream: block offsets, the header, the stream's size and status (emit_stream's rules)
__global__ __launch_bounds__(64) void ke_scan(CompressArgs A, const uint4 *recs, uint64_t rcap, EwBufs E) {
    const uint64_t s = blockIdx.x;
    const int lane = (int)threadIdx.x;
    int32_t H, done0;
    bool skip;
    ew_stream(A, s, H, done0, skip);
    if (skip) return;
    const int32_t n = (int32_t)(A.in_off[s + 1] - A.in_off[s]);
    uint8_t *out = A.out + A.out_off[s];
    const int64_t cap = (int64_t)(A.out_off[s + 1] - A.out_off[s]);
    const uint64_t pr = A.out_size[s];
    const int32_t m = (int32_t)((pr & 0xffffffffffffull) < rcap ? (pr & 0xffffffffffffull) : rcap);
    int err = (int)(pr >> 48);
    const bool spec = A.spec_mode != 0;
    uint64_t *inf = E.info + 4 * s;
    const bool refused = !spec && err != 0 && m == 0;  // by the parse, before its first record (emit_stream's rule)
    if (refused || (!spec && H > cap)) {  // not even the header
        if (lane == 0) {
            inf[0] = 0, inf[3] = 1;
            A.out_size[s] = 0;
            if (A.status) A.status[s] = refused ? err : EZ_ENOSPC;
        }
        return;
    }
    if (lane == 0 && !spec && H > 0) {
        const int32_t bsl = (int32_t)__builtin_ctzll((uint64_t)A.bs);
        const uint64_t hm = A.append_magic ? (0x141080797a616502ull << 8 | 0x80) : (0x80ull | 0x10ull << 8 | (uint64_t)bsl << 16);
        put_small(out, V16{hm, A.append_magic ? (uint64_t)bsl : 0ull}, (uint32_t)H);
    }
    const uint32_t nb = (uint32_t)((m + kEwRec - 1) / kEwRec);
    uint64_t run = (uint64_t)H;
    for (uint32_t b0 = 0; b0 < nb; b0 += 64) {
        const uint32_t b = b0 + (uint32_t)lane;
        const uint64_t v = b < nb ? E.bsum[s * E.nb + b] : 0;
        uint64_t incl = v;
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t u = (uint64_t)__shfl_up((long long)incl, d, 64);
            if (lane >= d) incl += u;
        }
        if (b < nb) E.bsum[s * E.nb + b] = run + incl - v;
        run += (uint64_t)__shfl((long long)incl, 63, 64);
    }
    if (lane != 0) return;
    const int32_t tail_at = m > 0 ? (int32_t)(recs[s * rcap + m - 1].x + recs[s * rcap + m - 1].y) : done0;
    inf[0] = (uint64_t)m, inf[1] = (uint64_t)tail_at, inf[2] = run, inf[3] = 0;
    if ((int64_t)run > cap) {  // ke_write's block at the crossing sets the size
        if (A.status) A.status[s] = err ? err : EZ_ENOSPC;
        inf[3] = 2;
        return;
    }
    uint64_t op = run;
    if (!err && tail_at < n) {  // the trailing literal (writer.go:324-329): its tag here, its bytes in ke_write
        const int32_t L = n - tail_at;
        int32_t ln = 0;
        const uint64_t lb = tag_bytes(0x00, L, &ln);
        if ((int64_t)op + ln + L > cap) {
            err = EZ_ENOSPC;
        } else {
            put_small(out + op, V16{lb, 0}, (uint32_t)ln);
            inf[3] = 4 | ((uint64_t)(op + ln) << 8);  // (the tail's bytes go to op + ln)
            op += ln + L;
        }
    }
    A.out_size[s] = op;
    if (A.status) A.status[s] = err;
}

__global__ __launch_bounds__(256) void ke_write(CompressArgs A, const uint4 *recs, uint64_t rcap, EwBufs E) {
    __shared__ uint64_t wsum[4];
    const uint64_t s = blockIdx.x / E.nb;
    const uint32_t b = blockIdx.x % E.nb;
    int32_t H, done0;
    bool skip;
    ew_stream(A, s, H, done0, skip);
    if (skip) return;
    const uint64_t *inf = E.info + 4 * s;
    if (inf[3] == 1) return;
    const int32_t m = (int32_t)inf[0];
    const uint8_t *lo = A.in, *hi = A.in + A.in_off[A.count];
    const uint8_t *p = A.in + A.in_off[s];
    uint8_t *out = A.out + A.out_off[s];
    const uint64_t cap = A.out_off[s + 1] - A.out_off[s];
    const int lane = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6);
    if ((int64_t)b * kEwRec < m) {
        const uint4 *rec = recs + s * rcap;
        // this thread's kEwPer consecutive records: sizes, then offsets by a block scan
        const int32_t r0 = (int32_t)b * kEwRec + (int32_t)threadIdx.x * kEwPer;
        uint64_t mine = 0;
        for (int32_t t = 0; t < kEwPer; t++) {
            int32_t la, L;
            if (r0 + t < m) mine += (uint64_t)ew_token(rec, r0 + t, done0, la, L);
        }
        uint64_t incl = mine;
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t u = (uint64_t)__shfl_up((long long)incl, d, 64);
            if (lane >= d) incl += u;
        }
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        uint64_t at = E.bsum[s * E.nb + b] + incl - mine;
        for (int v = 0; v < w; v++) at += wsum[v];
        for (int32_t t = 0; t < kEwPer; t++) {
            const int32_t r = r0 + t;
            const bool here = r < m;
            int32_t dk = 0, L = 0, T = 0;
            uint64_t lpos = 0;  // a long literal's output position
            bool longlit = false;
            if (here) {
                T = ew_token(rec, r, done0, dk, L);
                const uint4 v = rec[r];
                if (at + (uint64_t)T <= cap) {
                    uint8_t *d = out + at;
                    const bool lit = (v.w & 1) != 0 || L > 0;
                    int32_t ln = 0, tn = 0, on = 0;
                    const uint64_t lb = tag_bytes(0x00, L, &ln);
                    uint64_t tb = tag_bytes(0x80, (int32_t)v.y, &tn);
                    uint64_t ob = off_bytes((int32_t)v.z, (int32_t)v.y, &on);
                    if (v.y == 0) tb = ob = 0, tn = on = 0;
                    if (lit) {
                        put_small(d, V16{lb, 0}, (uint32_t)ln);
                        if (L >= kLongLit) {
                            longlit = true;
                            lpos = at + (uint64_t)ln;
                        } else {
                            copy_lane(d + ln, p + dk, L, lo, hi);
                        }
                    }
                    if (tn) {
                        const uint64_t c0 = tb | (ob << (8 * tn));
                        const uint64_t c1 = ob >> (64 - 8 * tn);
                        put_small(d + T - tn - on, V16{c0, c1}, (uint32_t)(tn + on));
                    }
                } else if (at <= cap) {  // the first token that does not fit: the output ends before it
                    A.out_size[s] = at;
                }
            }
            // long literals: the whole wave, one at a time (as emit_stream)
            for (uint64_t lm = __ballot(longlit); lm; lm &= lm - 1) {
                const int src = __builtin_ctzll(lm);
                const int32_t Ls = __shfl(L, src, 64), ds = __shfl(dk, src, 64);
                const uint64_t ts = (uint64_t)__shfl((long long)lpos, src, 64);
                for (int32_t q = 16 * lane; q < Ls; q += 16 * 64) {
                    const V16 v = ld16_in(p + ds + q, lo, hi);
                    if (q + 16 <= Ls) st16v(out + ts + q, v);
                    else put_small(out + ts + q, v, (uint32_t)(Ls - q));
                }
            }
            if (here) at += (uint64_t)T;
        }
    }
    // the trailing literal's bytes, by the stream's blocks in turn
    if (inf[3] & 4) {
        const int32_t n = (int32_t)(A.in_off[s + 1] - A.in_off[s]);
        const int32_t ta = (int32_t)inf[1];
        const int32_t L = n - ta;
        const uint64_t ts = inf[3] >> 8;
        for (int64_t q = ((int64_t)b * 256 + threadIdx.x) * 16; q < L; q += (int64_t)E.nb * 256 * 16) {
            const V16 v = ld16_in(p + ta + q, lo, hi);
            if (q + 16 <= L) st16v(out + ts + q, v);
            else put_small(out + ts + q, v, (uint32_t)(L - q));
        }
    }
}

// blocks of kEwRec records a stream's slot can hold
uint32_t ew_blocks(const CompressArgs &a) { return (uint32_t)((rec_cap(a) + kEwRec - 1) / kEwRec); }

}  // namespace

// the token writer, one wave per stream: k1_emit<false> for the 8-byte records of k1_parse and
// k1_lean, k1_emit<true> for 16-byte ones
hipError_t launch_emit(const CompressArgs &a, const uint64_t *recs, uint64_t rcap, bool wide_recs, hipStream_t st) {
    const unsigned grid = (unsigned)((a.count + 3) / 4);
    if (wide_recs) hipLaunchKernelGGL(k1_emit<true>, dim3(grid), dim3(256), 0, st, a, recs, rcap);
    else hipLaunchKernelGGL(k1_emit<false>, dim3(grid), dim3(256), 0, st, a, recs, rcap);
    return hipGetLastError();
}

// the chip-wide token writer's workspace (after K1L's records) and its launch: batches of at most
// 1,024 streams (C4s 36.9 -> 30.9 ms; C2's 4,096 streams keep k1_emit<true>, one wave per stream:
// 25.0 against 28.0 ms); EZ_K1E_WIDE=0 / 1 (experiment builds) forces either
uint64_t ew_bytes(const CompressArgs &a) { return up256(a.count * ew_blocks(a) * 8) + up256(a.count * 32); }
hipError_t launch_emit_wide(const CompressArgs &a, const uint4 *recs, uint64_t rcap, uint8_t *ws, hipStream_t st) {
    static const int wk = knob("EZ_K1E_WIDE", -1);
    const bool wide = wk < 0 ? a.count <= 1024 : wk != 0;
    if (!wide) return launch_emit(a, (const uint64_t *)recs, rcap, true, st);
    EwBufs E;
    E.nb = ew_blocks(a);
    E.bsum = (uint64_t *)ws;
    E.info = (uint64_t *)(ws + up256(a.count * E.nb * 8));
    const unsigned g = (unsigned)(a.count * E.nb);
    hipLaunchKernelGGL(ke_size, dim3(g), dim3(256), 0, st, a, recs, rcap, E);
    hipLaunchKernelGGL(ke_scan, dim3((unsigned)a.count), dim3(64), 0, st, a, recs, rcap, E);
    hipLaunchKernelGGL(ke_write, dim3(g), dim3(256), 0, st, a, recs, rcap, E);
    return hipGetLastError();
}

}  // namespace ez
