// ez_decompress_jump.hip — K2j: the decode of a few long streams with the whole chip.
//
// Reader.read (reader.go:143-216) is a chain twice over: every token starts where the previous one
// ends (readTag :218-270), and every copied byte reads output written before it (:173-201).  K2t
// runs both chains on one wave per stream, which leaves a batch of a few long streams (a Reader
// handle's one stream, C4's 64 buckets, 1 MiB streams) to a handful of waves on a 1,024-SIMD chip.
// K2j cuts both chains into data-parallel steps:
//
//  1. token starts (kj_spec, kj_verify, kj_fix): the compressed stream is cut into 1 KiB chunks; a
//     lane per chunk parses speculatively from kJWarm bytes before the chunk and records the
//     positions it visits inside it (a bitmap) and where it leaves it.  A wrong start parses
//     garbage, but its chain meets the true one within a few tokens (median ~110 bytes on the log
//     streams; 99 % within 1 KiB), after which both are the same chain, so the warm-up has usually
//     met it before the chunk starts.  kj_verify (a lane per chunk, all in parallel) takes chunk j's
//     entry to be chunk j-1's speculative exit and walks the true chain from it until it meets a
//     recorded position (the chunk's exit is then the speculative one) or leaves the chunk.
//     kj_fix (a wave per stream) finds, 64 chunks per step, the first chunk whose assumed entry
//     differs from its predecessor's true exit and re-walks only that chunk (rare); an entry past a
//     chunk (inside a long token) skips to the chunk it lies in.
//  2. tokens (kj_tok, kj_scan, kj_place): a lane per chunk walks the true chain from its entry
//     once, checks every form (k2_scan, ez_k2_parse.h) and writes a chunk-local record per token
//     (output position from the chunk's start, length, distance or input position), its token and
//     output counts, the longest distance and its Breaks; a wave per stream scans the chunks'
//     counts into token and output positions and validates the stream as K2t does (one MetaReset
//     before any output, the window set before the first token, every distance within the window,
//     the output within the slot); kj_place moves each chunk's records into the stream's array.
//  3. bytes (kj_expand): a thread per 16 output bytes finds its tokens (a binary search over the
//     stream's records), writes literal bytes and zero regions, and for every copied byte p a
//     pointer ptr[p] = p - D (a marker for bytes before the stream start: the fresh window's zeros,
//     SURVEY A.12; a Reader's continuation points into the history placed before out_off[0]);
//     literal, zero and history bytes point at themselves.
//  4. copies (kj_jump): pointer jumping, ptr[p] = ptr[ptr[p]] over all bytes, until every pointer
//     names a literal byte, a zero byte or the zero marker: ceil(log2(chain depth)) passes, each a
//     sequential read and a gather that stays mostly local (copy distances are short).  Passes
//     after the one that changed nothing return at once (the launcher queues a fixed number, so
//     nothing waits on the host).
//  5. kj_gather writes every copied byte from its resolved source; kj_final reports each stream
//     (out_size, status, Break positions, a Reader's end state) or hands it to the exact decoder.
//
// Continuation (DecompressArgs.c_on, a NewReader's read-ahead, ez_reader.hip stream_ahead): one stream
// whose history (c_hist bytes) sits before out_off[0]; the chain stops before a token the input ends
// inside of, a literal whose body runs past the input is output as far as it goes, and the end state
// says where the input was left.
//
// Streams K2j cannot take as a whole (an error, a form k2_scan hands over, a MetaReset after output,
// a slot too small) go to the exact decoder (ez_decompress.hip), which recomputes them from the start.
//
// Extent hints (ez_batch.in_bytes / out_bytes): the workspace is sized from them, so kj_init checks
// them against the real offsets; a batch larger than its hints goes to the exact decoder as a whole
// (kj_guarded).  Over-stated hints only make the workspace larger; one hint alone counts as none.
#include <hip/hip_runtime.h>

#include "ez_cache.h"
#include "ez_k2_jump.h"
#include "ez_wave.h"

namespace ez {
namespace {

// The guard: the batch's real extents exceed the ones its workspace was sized from (an under-stated
// ez_batch.in_bytes / out_bytes).  kj_init sets it; every later kernel but kj_final returns at once,
// so nothing indexes the workspace by the real offsets, and kj_final queues every stream for the
// exact decoder.
__device__ __forceinline__ bool kj_guarded(const JWork &W) { return W.pass[kJPasses] != 0; }

// The walks of kj_spec / kj_verify / kj_tok read their chunk's tokens from LDS: a block's 64 chunks are
// consecutive in the batch's input (a stream's chunks follow each other, and so do the streams), so
// the block stages the bytes from its first chunk's start to 16 past its last chunk's end with
// coalesced 16-byte loads, and every token step is then an LDS read instead of a dependent global
// load (DESIGN §4 K2j has the times).  The walks themselves are ez_k2_jump.h's, over JStage as the accessor.
struct JStage {
    uint8_t *lds;
    uint64_t base;  // batch offset of lds[0]
    __device__ __forceinline__ V16 operator()(uint64_t y) const {  // 16 bytes at batch offset y (staged)
        const uint8_t *q = lds + (y - base);
        typedef uint64_t __attribute__((aligned(1))) u64u;
        return V16{*(const u64u *)q, *(const u64u *)(q + 8)};
    }
};
// stage [first chunk's start, last chunk's end + 16) of the batch (zeros past its end); every lane of
// the block calls it (a lane without a chunk passes live = false); returns the block's staging
__device__ __forceinline__ JStage kj_stage(const DecompressArgs &A, bool live, uint64_t start, uint64_t end, uint8_t *lds) {
    __shared__ uint64_t ext[2];
    if (threadIdx.x == 0) {
        ext[0] = ~0ull;
        ext[1] = 0;
    }
    __syncthreads();
    if (live) {
        atomicMin((unsigned long long *)&ext[0], (unsigned long long)start);
        atomicMax((unsigned long long *)&ext[1], (unsigned long long)end);
    }
    __syncthreads();
    const uint64_t base = ext[0], stop = ext[1] + 16;
    const KjBatch in{A.in, A.in_off[A.count]};
    if (base < stop) {
        for (uint64_t o = (uint64_t)threadIdx.x * 16; base + o < stop; o += (uint64_t)blockDim.x * 16) {
            const V16 v = in(base + o);
            typedef uint64_t __attribute__((aligned(8))) u64a;
            *(u64a *)(lds + o) = v.lo;
            *(u64a *)(lds + o + 8) = v.hi;
        }
    }
    __syncthreads();
    return JStage{lds, base};
}
// ---- 0: chunks per stream
__global__ __launch_bounds__(1024) void kj_init(DecompressArgs A, JWork W) {
    __shared__ uint32_t part[1024];
    const uint32_t t = threadIdx.x;
    uint32_t carry = 0;
    // the real extents against the ones the workspace holds (every thread reads the same four offsets);
    // past them, only head and cbase (sized by count) are written: every stream handed over, no chunks
    const bool over = A.in_off[A.count] - A.in_off[0] > W.in_ext || A.out_off[A.count] - A.out_off[0] > W.out_ext;
    if (over && t == 0) W.pass[kJPasses] = 1;
    for (uint32_t base = 0; base < (uint32_t)A.count; base += 1024) {
        const uint32_t s = base + t;
        uint32_t nch = 0;
        if (s < A.count && over) {
            JHead h{};
            h.state = 1;
            h.bsl = -1;
            W.head[s] = h;
        } else if (s < A.count) {
            const uint64_t nb = A.in_off[s + 1] - A.in_off[s];
            const uint64_t cap = A.out_off[s + 1] - A.out_off[s];
            nch = nb == 0 ? 1u : (uint32_t)((nb + W.jc - 1) / W.jc);
            JHead h{};
            // (pointers are 32-bit offsets from the batch's first output slot, rounded down to 16 bytes)
            h.state = (nb >= (1ull << 31) || cap >= (1ull << 32) - 2 || A.out_off[s + 1] - jg0(A) >= (1ull << 32) - 2) ? 1u : 0u;
            h.bsl = -1;
            h.tstop = (int32_t)(nb < (1ull << 31) ? nb : 0);
            h.tj = 0;
            h.tL = 0;
            h.nchunk = nch;
            W.head[s] = h;
        }
        part[t] = nch;
        __syncthreads();
        for (uint32_t d = 1; d < 1024; d <<= 1) {  // inclusive scan
            const uint32_t v = t >= d ? part[t - d] : 0;
            __syncthreads();
            part[t] += v;
            __syncthreads();
        }
        if (s < A.count) {
            const uint32_t c0 = carry + part[t] - nch;
            W.cbase[s] = c0;
            W.head[s].chunk0 = c0;
        }
        carry += part[1023];
        __syncthreads();
    }
    if (t == 0) W.cbase[A.count] = carry;
}

// ---- 1a: speculative parse of each chunk (from kJWarm bytes before it): the positions it visits in the
// chunk, and its exit
__global__ __launch_bounds__(64) void kj_spec(DecompressArgs A, JWork W) {
    __shared__ uint32_t bm[64][kJW + 1];
    __shared__ __attribute__((aligned(16))) uint8_t stage[kJStage];
    if (kj_guarded(W)) return;
    const uint32_t lane = threadIdx.x;
    const uint32_t c = blockIdx.x * 64 + lane;
    const KjChunk K = kj_chunk(c, W.cbase, (uint32_t)A.count, A.in_off, W.head, W.jc);
    const JStage S = kj_stage(A, K.live, K.b0 + (uint64_t)kj_warm0(K.c0), K.b0 + (uint64_t)K.ce, stage);
    if (!K.live) return;
    const int32_t p = kj_spec_walk(S, K.b0, K.c0, K.ce, bm[lane]);
    uint32_t *g = W.bits + (uint64_t)c * kJW;
    for (int k = 0; k < kJW; k++) g[k] = bm[lane][k];
    W.sexit[c] = (uint32_t)p;
}

// ---- 1b: the true entry of every chunk.  Chunk c's entry is its predecessor's speculative exit when
// the predecessor's speculative chain merged with the true chain inside it (a wrong start meets the
// true chain within ~110 bytes on the logs, 99 % within 1 KiB); every chunk checks that at once
// (kj_verify: thread per chunk, walking the true chain from that entry until a position its own
// speculative parse visited -- its speculative exit is then its true exit -- or its end), and a wave
// per stream then redoes, in order, only the chunks whose predecessor did not merge (kj_fix).
// texit[c]: chunk c's true exit given that entry; entry[c]: the entry the check assumed
__global__ __launch_bounds__(64) void kj_verify(DecompressArgs A, JWork W) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kJStage];
    if (kj_guarded(W)) return;
    const uint32_t c = blockIdx.x * 64 + threadIdx.x;
    const KjChunk K = kj_chunk(c, W.cbase, (uint32_t)A.count, A.in_off, W.head, W.jc);
    const JStage S = kj_stage(A, K.live, K.b0 + (uint64_t)K.c0, K.b0 + (uint64_t)K.ce, stage);
    if (!K.live) return;
    const int32_t a = K.c0 == 0 ? 0 : (int32_t)W.sexit[c - 1];  // (chunk 0 starts at the stream's start, on the true chain)
    W.entry[c] = (uint32_t)a;
    // (the true exit; kj_tok overwrites cnt with the token count)
    W.cnt[c] = (uint32_t)kj_follow(S, K.b0, a, K.c0, K.ce, W.bits + (uint64_t)c * kJW, W.sexit + c);
}

__global__ __launch_bounds__(64) void kj_fix(DecompressArgs A, JWork W) {
    if (kj_guarded(W)) return;
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    JHead &H = W.head[s];
    if (H.state) return;
    const int32_t nb = (int32_t)(A.in_off[s + 1] - A.in_off[s]);
    const uint32_t c00 = H.chunk0, nch = H.nchunk;
    uint32_t *texit = W.cnt;
    // chunks [0, k) are right; chunk j's entry is right iff its predecessor's true exit is the
    // speculative exit it assumed.  The true exit of the chunk fixed last is kept in a register
    // (fx_at, fx_val): this kernel's own stores are not read back.
    uint32_t k = 1, fx_at = ~0u;
    int32_t fx_val = 0;
    while (k < nch) {
        const uint32_t j = k + lane;
        bool bad = false;
        if (j < nch) {
            const uint32_t tx = j - 1 == fx_at ? (uint32_t)fx_val : texit[c00 + j - 1];
            bad = tx != W.sexit[c00 + j - 1];
        }
        const uint64_t m = __ballot(bad);
        if (m == 0) {
            k += 64;
            continue;
        }
        const uint32_t jf = k + (uint32_t)__builtin_ctzll(m);  // the first chunk entered wrongly
        const int32_t e = jf - 1 == fx_at ? fx_val : (int32_t)texit[c00 + jf - 1];  // its true entry
        // the chunks before the one that holds e pass it through
        const uint32_t kw = kj_holder(e, jf, nb, nch, W.jc);
        for (uint32_t x = jf + lane; x < kw; x += 64) {
            W.entry[c00 + x] = (uint32_t)e;
            texit[c00 + x] = (uint32_t)e;
        }
        if (kw >= nch) {
            fx_at = nch - 1;
            fx_val = e;
            break;
        }
        // chunk kw holds e: the true chain from there (one lane; rare), on global memory
        int32_t x = 0;
        if (lane == 0) {
            const int32_t cs = (int32_t)kw * W.jc, ce = cs + W.jc < nb ? cs + W.jc : nb;
            x = kj_follow(KjBatch{A.in, A.in_off[A.count]}, A.in_off[s], e, cs, ce, W.bits + (uint64_t)(c00 + kw) * kJW, W.sexit + c00 + kw);
            W.entry[c00 + kw] = (uint32_t)e;
            texit[c00 + kw] = (uint32_t)x;
        }
        fx_at = kw;
        fx_val = __shfl(x, 0);
        k = kw + 1;
    }
    const int32_t last = nch - 1 == fx_at ? fx_val : (int32_t)texit[c00 + nch - 1];
    if (lane == 0 && kj_chain_bad(last, nb, A.c_on != 0)) H.state = 1;
}

// ---- 2a: the true chain of each chunk, parsed once: tokens, output bytes, forms and metas, a record
// per token (chunk-local: output positions from the chunk's start; kj_place moves them into the
// stream's array once the chunks' positions are known), the longest distance, Break positions
__global__ __launch_bounds__(64) void kj_tok(DecompressArgs A, JWork W) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kJStage];
    if (kj_guarded(W)) return;
    const uint32_t c = blockIdx.x * 64 + threadIdx.x;
    const KjChunk K = kj_chunk(c, W.cbase, (uint32_t)A.count, A.in_off, W.head, W.jc);
    const JStage S = kj_stage(A, K.live, K.b0 + (uint64_t)K.c0, K.b0 + (uint64_t)K.ce, stage);
    if (!K.live) return;
    const auto brk = [&](uint64_t out) {  // (one-stream batches) a Break: (chunk, local position)
        const uint64_t at = atomicAdd((unsigned long long *)A.breaks, 1ull);
        if (at < A.breaks_cap) A.breaks[1 + at] = ((uint64_t)c << 32) | (out & 0xffffffffull);
    };
    const KjSum r = kj_tok_walk(S, K.b0, K.nb, K.ce, (int32_t)W.entry[c], k2_lim32(A.block_size_limit), A.block_size_limit, A.c_on != 0,
                                W.ltok + (uint64_t)c * kJRec, W.head[K.s], A.breaks != nullptr, brk);
    W.cnt[c] = r.n;
    W.cout[c] = r.out;
    W.cflag[c] = r.fl;
    W.cmaxd[c] = r.maxd;
}

// ---- 2b: token and output positions of the chunks; the stream's checks (wave per stream)
__global__ __launch_bounds__(64) void kj_scan(DecompressArgs A, JWork W, uint64_t *tok_alloc) {
    if (kj_guarded(W)) return;
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    JHead &H = W.head[s];
    if (H.state) return;
    const uint32_t c00 = H.chunk0, nch = H.nchunk;
    uint64_t tcarry = 0, ocarry = 0;
    int32_t bsl = A.c_on ? A.c_bsl : -1;  // (a Reader's read-ahead: the window its stream has set)
    bool bad = false;
    uint32_t maxd = 0;
    for (uint32_t k = 0; k < nch; k += 64) {
        const uint32_t j = k + lane;
        const bool mine = j < nch;
        const uint64_t n = mine ? W.cnt[c00 + j] : 0, o = mine ? W.cout[c00 + j] : 0;
        const uint32_t fl = mine ? W.cflag[c00 + j] : 0;
        maxd = max(maxd, wmax_u32(mine ? W.cmaxd[c00 + j] : 0));
        const uint64_t in = wscan_add_u64(n), io = wscan_add_u64(o);
        const uint64_t obefore = ocarry + io - o;
        if (mine) {
            W.ctbase[c00 + j] = tcarry + in - n;
            W.cobase[c00 + j] = obefore;
        }
        // (the window a stream's MetaResets set is the last one's)
        if (__ballot(mine && kj_chunk_bad(fl, obefore, A.c_on && A.c_pos0 != 0))) bad = true;
        const uint64_t rm = __ballot(mine && (fl & kJFReset));
        if (rm) bsl = (int32_t)((__shfl(fl, 63 - __builtin_clzll(rm)) >> 8) & 0xff);
        tcarry = __shfl(tcarry + in, 63);
        ocarry = __shfl(ocarry + io, 63);
    }
    if (lane != 0) return;
    if (!bad) {
        bool nospace;
        bad = kj_stream_bad(ocarry, bsl, maxd, A.out_off[s + 1] - A.out_off[s], A.c_on != 0, H, (int32_t)(A.in_off[s + 1] - A.in_off[s]), nospace);
        if (nospace && A.end_state) A.end_state[0] = -2;  // (a caller that sizes its slot grows it and retries)
    }
    if (!bad) {
        const uint64_t t0 = atomicAdd((unsigned long long *)tok_alloc, (unsigned long long)tcarry);
        if (t0 + tcarry > W.tok_cap) bad = true;
        H.tok0 = t0;
    }
    H.bsl = bsl;
    H.total = ocarry;
    H.ntok = tcarry;
    if (bad) H.state = 1;
}

// ---- 2c: the chunks' records into the stream's array, positions from the stream's start (block per chunk)
__global__ __launch_bounds__(64) void kj_place(DecompressArgs A, JWork W) {
    if (kj_guarded(W)) return;
    const uint32_t c = blockIdx.x;
    if (c >= W.cbase[A.count]) return;
    const uint32_t s = last_le(W.cbase, (uint32_t)A.count, c);
    const JHead &H = W.head[s];
    if (H.state) return;
    const JTok *src = W.ltok + (uint64_t)c * kJRec;
    JTok *dst = W.tok + H.tok0 + W.ctbase[c];
    const uint32_t n = W.cnt[c], ob = (uint32_t)W.cobase[c];
    for (uint32_t k = threadIdx.x; k < n; k += 64) {
        JTok t = src[k];
        t.dst += ob;
        dst[k] = t;
    }
}

// ---- 3: literal and zero bytes, and a pointer for every copied byte (thread per 16 output bytes)
// (kj_piece, ez_k2_jump.h: the bytes and pointers of up to 16 output bytes of one stream)
__global__ __launch_bounds__(256) void kj_expand(DecompressArgs A, JWork W) {
    if (kj_guarded(W)) return;
    const uint64_t ob = A.out_off[0], g0 = jg0(A), end = A.out_off[A.count];
    const uint64_t hst = A.c_on ? ob - A.c_hist : ob;  // (c_on) the history [hst, ob): final bytes, pointing at themselves
    for (uint64_t g = g0 + ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16; g < end; g += (uint64_t)gridDim.x * blockDim.x * 16) {
        // the stream of the piece's first byte of the batch
        const uint64_t x0 = g > ob ? g : ob;
        uint32_t s = last_le(A.out_off, (uint32_t)A.count, x0);
        const uint64_t ge = g + 16 < end ? g + 16 : end;
        const JHead H = W.head[s];
        if (!H.state && A.out_off[s] <= g && A.out_off[s] + H.total >= g + 16 && ge == g + 16) {
            // the common case: the 16 bytes all in stream s's output, one store of each kind
            uint32_t by[4] = {0, 0, 0, 0}, pt[16];
            kj_piece(A, W, H, s, g, 16, g0, by, pt);
            *(uint4 *)(A.out + g) = make_uint4(by[0], by[1], by[2], by[3]);  // (copied bytes: kj_gather)
            uint32_t *pp = W.ptr + (g - g0);
#pragma unroll
            for (int q = 0; q < 4; q++) *(uint4 *)(pp + 4 * q) = make_uint4(pt[4 * q], pt[4 * q + 1], pt[4 * q + 2], pt[4 * q + 3]);
            continue;
        }
        // a piece at a slot's end (or before the batch's first slot): each stream's output bytes in it,
        // byte by byte
        for (uint64_t y = g > hst ? g : hst; y < ob && y < ge; y++) W.ptr[y - g0] = (uint32_t)(y - g0);
        for (uint64_t x = x0; x < ge;) {
            while (s + 1 < (uint32_t)A.count && A.out_off[s + 1] <= x) s++;
            const JHead Hs = W.head[s];
            const uint64_t ob2 = A.out_off[s] + Hs.total, se = A.out_off[s + 1] < ge ? A.out_off[s + 1] : ge;
            if (!Hs.state && x < ob2) {
                const uint32_t n = (uint32_t)((ob2 < se ? ob2 : se) - x);
                uint32_t by[4] = {0, 0, 0, 0}, pt[16];
                kj_piece(A, W, Hs, s, x, n, g0, by, pt);
                for (uint32_t k = 0; k < n; k++) {
                    A.out[x + k] = (uint8_t)(by[k >> 2] >> (8 * (k & 3)));
                    W.ptr[x - g0 + k] = pt[k];
                }
            }
            x = se;
        }
    }
}

// ---- 4: one pointer-jumping pass (returns at once when the pass before changed nothing)
__global__ __launch_bounds__(256) void kj_jump(DecompressArgs A, JWork W, int pass) {
    if (kj_guarded(W) || (pass > 0 && W.pass[pass - 1] == 0)) return;
    const uint64_t end = A.out_off[A.count] - jg0(A);  // (ptr counts from g0)
    bool changed = false;
    for (uint64_t g = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; g < end; g += (uint64_t)gridDim.x * blockDim.x * 4) {
        uint4 v = g + 4 <= end ? *(const uint4 *)(W.ptr + g) : make_uint4(kJGap, kJGap, kJGap, kJGap);
        if (g + 4 > end)
            for (uint64_t k = g; k < end; k++) (&v.x)[k - g] = W.ptr[k];
        uint32_t *e = &v.x;
        // the four gathers issued together (a pointer to itself or a marker is final)
        uint32_t r[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t q = e[k];
            r[k] = q >= kJZero || q == (uint32_t)(g + k) ? q : W.ptr[q];
        }
        bool any = false;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            any |= r[k] != e[k];
            e[k] = r[k];
        }
        if (any) {
            changed = true;
            if (g + 4 <= end) *(uint4 *)(W.ptr + g) = v;
            else
                for (uint64_t k = g; k < end; k++) W.ptr[k] = e[k - g];
        }
    }
    if (__ballot(changed) != 0 && (threadIdx.x & 63) == 0) W.pass[pass] = 1;
}

// ---- 5a: every copied byte from its resolved source
__global__ __launch_bounds__(256) void kj_gather(DecompressArgs A, JWork W) {
    if (kj_guarded(W)) return;
    const uint64_t g0 = jg0(A), end = A.out_off[A.count] - g0;
    uint8_t *o = A.out + g0;
    for (uint64_t g = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; g < end; g += (uint64_t)gridDim.x * blockDim.x * 4) {
        for (uint64_t x = g; x < g + 4 && x < end; x++) {
            const uint32_t q = W.ptr[x];
            if (q == kJGap || q == (uint32_t)x) continue;
            o[x] = q == kJZero ? (uint8_t)0 : o[q];
        }
    }
}

// ---- 5b: results, or the stream to the exact decoder; a one-stream batch's Break positions from
// (chunk, local position) to the stream's output positions.  Under the guard every head says handed
// over (kj_init), so only head and the slow list, both sized by count, are touched
__global__ __launch_bounds__(256) void kj_final(DecompressArgs A, JWork W) {
    if (A.breaks && A.count == 1 && blockIdx.x == 0 && !W.head[0].state) {
        const uint64_t nbrk = A.breaks[0] < A.breaks_cap ? A.breaks[0] : A.breaks_cap;
        for (uint64_t k = threadIdx.x; k < nbrk; k += blockDim.x) {
            const uint64_t v = A.breaks[1 + k];
            A.breaks[1 + k] = W.cobase[v >> 32] + (v & 0xffffffffull);
        }
    }
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < A.count; s += (uint64_t)gridDim.x * blockDim.x) {
        const JHead H = W.head[s];
        if (H.state) {
            const uint32_t at = atomicAdd(&A.slow[0], 1u);
            A.slow[1 + at] = (uint32_t)s;
            continue;
        }
        A.out_size[s] = H.total;
        if (A.status) A.status[s] = EZ_OK;
        if (A.end_state) {  // (one MetaReset, before any output: r.pos is the output since the start)
            A.end_state[0] = H.bsl < 0 ? 0 : (int64_t)1 << H.bsl;
            A.end_state[1] = (int64_t)H.total;
            if (A.c_on) {
                A.end_state[2] = H.tstop;
                A.end_state[3] = H.tj;
                A.end_state[4] = H.tL;
            }
        }
    }
}

}  // namespace

// K2j's workspaces per (device, HIP stream) (ez_cache.h)
DevCache &jump_cache() {
    static DevCache *c = new DevCache();  // (never destroyed: no hipFree after the runtime's teardown)
    return *c;
}

// Streams K2j takes: a batch of at most 1,024 streams (slots below 4 GiB in all)
bool jump_applies(const DecompressArgs &a) { return a.count >= 1 && a.count <= 1024; }

uint64_t jump_workspace_bytes(uint64_t count, uint64_t in_total, uint64_t out_total) {
    return JLayout(count, in_total, out_total).total;
}

hipError_t batch_extents(const DecompressArgs &a, hipStream_t st, uint64_t *in_bytes, uint64_t *out_bytes) {
    // the caller's hints only as a pair: one alone says nothing about the other extent, so it counts as
    // unknown (kj_init checks the pair against the real offsets: a wrong hint costs speed, not memory)
    if (a.in_bytes && a.out_bytes) {
        *in_bytes = a.in_bytes;
        *out_bytes = a.out_bytes;
        return hipSuccess;
    }
    uint64_t ext[4] = {0, 0, 0, 0};  // (the offsets may be a view into a larger batch's: absolute)
    hipError_t e;
    if ((e = hipMemcpyAsync(&ext[0], a.in_off, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(&ext[1], a.in_off + a.count, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(&ext[2], a.out_off, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(&ext[3], a.out_off + a.count, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    *in_bytes = ext[1] - ext[0];
    *out_bytes = ext[3] - ext[2];
    return hipSuccess;
}

hipError_t launch_decompress_jump(const DecompressArgs &a, hipStream_t st) {
    // the batch's input and output extents (the caller's hints, else one read back): the workspace is
    // sized from them; the ptr array covers out_off[0] rounded down to 16 bytes .. out_off[count]
    uint64_t in_total = 0, out_bytes = 0;
    hipError_t e = batch_extents(a, st, &in_total, &out_bytes);
    if (e != hipSuccess) return e;
    const uint64_t out_total = out_bytes + (a.c_on ? a.c_hist : 0) + 16;  // (+ the history a continuation reads)
    const JLayout Y(a.count, in_total, out_total);
    // the caller's workspace when it gives one large enough, else this (device, stream)'s (its lease
    // is held through the launches: another host thread growing it meanwhile would free it under them)
    CacheLease lease;
    uint8_t *w = (uint8_t *)a.jws;
    if (!w || a.jws_cap < Y.total) {
        int dev = 0;
        if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
        lease = jump_cache().acquire(dev, (void *)st);
        if (!lease->ensure(Y.total)) return hipErrorOutOfMemory;  // (the caller decodes the batch on K2t)
        w = (uint8_t *)lease->p;
    }
    const JWork W = Y.bind(w, in_total, out_bytes);
    uint64_t *tok_alloc = (uint64_t *)(W.pass + kJPasses + 2);
    if ((e = hipMemsetAsync(W.pass, 0, 8 * (kJPasses + 2), st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(W.ptr, 0xff, 4 * out_total + 16, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(kj_init, dim3(1), dim3(1024), 0, st, a, W);
    const unsigned cgrid = (unsigned)((Y.chunks + 63) / 64);
    hipLaunchKernelGGL(kj_spec, dim3(cgrid), dim3(64), 0, st, a, W);
    hipLaunchKernelGGL(kj_verify, dim3(cgrid), dim3(64), 0, st, a, W);
    hipLaunchKernelGGL(kj_fix, dim3((unsigned)a.count), dim3(64), 0, st, a, W);
    hipLaunchKernelGGL(kj_tok, dim3(cgrid), dim3(64), 0, st, a, W);
    hipLaunchKernelGGL(kj_scan, dim3((unsigned)a.count), dim3(64), 0, st, a, W, tok_alloc);
    hipLaunchKernelGGL(kj_place, dim3((unsigned)Y.chunks), dim3(64), 0, st, a, W);
    const uint64_t pieces = (out_total + 15) / 16;  // (out_total: the batch's output and the alignment slack)
    const unsigned egrid = (unsigned)(pieces / 256 + 1 < 8192 ? pieces / 256 + 1 : 8192);
    hipLaunchKernelGGL(kj_expand, dim3(egrid), dim3(256), 0, st, a, W);
    const uint64_t quads = (out_total + 3) / 4;
    const unsigned jgrid = (unsigned)(quads / 256 + 1 < 8192 ? quads / 256 + 1 : 8192);
    // every pass at least halves the longest pointer chain, and a chain is shorter than the output:
    // ceil(log2(output)) + 1 passes finish it (the ones after it return at once)
    int passes = 1;
    while (passes < kJPasses && ((uint64_t)1 << (passes - 1)) < out_total) passes++;
    for (int k = 0; k < passes; k++) hipLaunchKernelGGL(kj_jump, dim3(jgrid), dim3(256), 0, st, a, W, k);
    hipLaunchKernelGGL(kj_gather, dim3(jgrid), dim3(256), 0, st, a, W);
    hipLaunchKernelGGL(kj_final, dim3((unsigned)((a.count + 255) / 256)), dim3(256), 0, st, a, W);
    return hipGetLastError();
}

}  // namespace ez
