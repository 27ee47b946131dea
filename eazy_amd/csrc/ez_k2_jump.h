// ez_k2_jump.h — the per-chunk and per-stream steps of K2j (ez_decompress_jump.hip: the decode of a
// few long streams with the whole chip), its workspace and its layout.
//
// The steps are functions over a byte accessor at(y): the 16 bytes at batch offset y, zeros past the
// batch's end.  The kernels pass their LDS staging (JStage, kj_spec / kj_verify / kj_tok) or the
// batch in global memory (KjBatch, kj_fix); tools/k2_jump_check.hip passes a staging buffer on the
// host and runs every stage over the same source against the oracle.
//   kj_chunk       a chunk's view: its stream, its bytes [c0, ce) of it, whether K2j still decodes it;
//   kj_spec_walk   the speculative walk from kJWarm bytes before the chunk: the positions visited in
//                  the chunk (a bitmap) and the exit;
//   kj_follow      from an entry to the first recorded position (the exit is then the speculative
//                  one), else the chunk's end; an entry at or past the end passes through;
//   kj_holder, kj_chain_bad   kj_fix's two decisions around kj_follow;
//   kj_tok_walk    the true chain with the full k2_scan: records, counts, flags, the continuation's stop;
//   kj_chunk_bad, kj_stream_bad   kj_scan's checks, per chunk and on the scanned totals;
//   kj_piece       pointers and bytes of up to 16 output bytes.
// What K2j shares with K2z (ez_k2_size.h): kz_reset_bad and kz_end_ok.  K2z's walks (kz_spec,
// kz_verify, kz_sum) are the same chain over a compile-time chunk size and a per-stream staging with
// zeros past the stream (kz_clamp_pad); K2j's run over the runtime chunk size JWork.jc and a staging of
// the batch, in which the next stream's bytes follow a stream's end, and write records.
#pragma once

#include "ez_internal.h"
#include "ez_k2_size.h"

namespace ez {

constexpr int32_t kJC = 1024;                        // compressed bytes per chunk at most (JWork.jc: 1,024 or 256)
constexpr int32_t kJW = kJC / 32;                    // bitmap words per chunk
constexpr uint32_t kJGap = 0xffffffffu;              // ptr: not a byte of any stream's output
constexpr uint32_t kJZero = 0xfffffffeu;             // ptr: a zero byte of the history before the stream
constexpr uint32_t kJCopy = 0x80000000u;             // JTok.kd: a copy (distance in the low bits; 0: zero region)
constexpr int kJPasses = 34;                         // pointer-jumping passes at most (chains up to 2^34)
constexpr uint32_t kJRec = kJC / 2 + 2;              // token records of a chunk at most (a token takes >= 2 bytes)
// kj_spec starts each chunk's speculative parse kJWarm bytes before it (positions before the chunk are
// not recorded), so that its chain has usually met the true one by the chunk's start: kj_verify's
// walks then end at their first step and kj_fix has (almost) nothing to redo
constexpr int32_t kJWarm = 256;
constexpr int32_t kJStage = 64 * kJC + kJWarm + 32;  // LDS bytes of a block's staged input

struct JHead {
    uint32_t chunk0, nchunk;  // the stream's chunks
    uint32_t state;           // 0: K2j decodes it; 1: handed over
    int32_t bsl;              // log2 of the window (MetaReset)
    uint64_t total;           // output bytes
    uint64_t ntok;            // token records
    uint64_t tok0;            // its first record
    // (c_on) where the chain stops: the input consumed by whole tokens, and a literal starting there
    // whose body runs past the input (its header length, its length; 0: none)
    int32_t tstop, tj;
    int64_t tL;
};

struct JTok {
    uint32_t dst, L, kd, src;  // output position, length, kJCopy | distance (or 0: literal), literal's input position
};

struct JWork {
    JHead *head;
    uint32_t *cbase;    // count+1: first chunk of each stream (and the total)
    uint32_t *entry, *sexit, *bits;
    uint32_t *cnt;      // tokens of a chunk's true chain
    uint64_t *cout;     // output bytes of a chunk
    uint32_t *cflag;    // kJF* bits, bits 8-15: the chunk's last MetaReset
    uint64_t *ctbase, *cobase;
    JTok *tok;
    uint64_t tok_cap;
    JTok *ltok;         // kj_tok's records, chunk-local (kJRec per chunk, dst from the chunk's output start)
    uint32_t *cmaxd;    // the longest copy distance of a chunk
    uint32_t *ptr;
    uint32_t *pass;     // [kJPasses]: the pass changed something; [kJPasses]: the guard (kj_init); then token records allocated
    int32_t jc;         // compressed bytes per chunk (jchunk)
    // the input and output extents the workspace was sized from (the caller's hints, or read back):
    // kj_init checks the real offsets against them
    uint64_t in_ext, out_ext;
};

// Chunks of 256 bytes for batches of at most 96 KiB of input (a Reader's refill of ~64 KiB: four
// times the lanes, each walk a quarter as long -- one wave of 1 KiB chunks was the refill's critical
// path: 0.60 -> 0.51 ms; C++ NewReader over 64 KiB pieces 143 -> 200 - 208 MiB/s), 1 KiB above (at
// 122 / 244 KiB, 256-byte chunks measured 0.85 / 1.03 against 0.82 / 0.66 ms: the per-stream scan and
// fix over four times the chunks outweigh the shorter walks)
inline int32_t jchunk(uint64_t in_total) { return in_total <= (96ull << 10) ? 256 : kJC; }

// the workspace layout of a batch (in_total / out_total: the end offsets in_off[count], out_off[count])
struct JLayout {
    uint64_t chunks, tok_cap;
    size_t o_head, o_cbase, o_entry, o_sexit, o_bits, o_cnt, o_cout, o_cflag, o_ctb, o_cob, o_tok, o_ltok, o_maxd, o_ptr, o_pass, total;
    JLayout(uint64_t count, uint64_t in_total, uint64_t out_total) {
        chunks = in_total / (uint64_t)jchunk(in_total) + 2 * count + 2;
        tok_cap = in_total / 2 + chunks + 16;  // (a token takes >= 2 input bytes; one may start in each chunk's last byte)
        size_t off = 0;
        auto take = [&](size_t n) {
            const size_t o = off;
            off += (n + 255) & ~(size_t)255;
            return o;
        };
        o_head = take(sizeof(JHead) * count), o_cbase = take(4 * (count + 1)), o_entry = take(4 * chunks), o_sexit = take(4 * chunks),
        o_bits = take(4 * kJW * chunks), o_cnt = take(4 * chunks), o_cout = take(8 * chunks), o_cflag = take(4 * chunks),
        o_ctb = take(8 * chunks), o_cob = take(8 * chunks), o_tok = take(sizeof(JTok) * tok_cap),
        o_ltok = take(sizeof(JTok) * kJRec * chunks), o_maxd = take(4 * chunks), o_ptr = take(4 * out_total + 16),
        o_pass = take(8 * (kJPasses + 2));
        total = off;
    }
    // the workspace at w (total bytes) of a batch of in_ext input and out_ext output bytes
    JWork bind(uint8_t *w, uint64_t in_ext, uint64_t out_ext) const {
        return JWork{(JHead *)(w + o_head),    (uint32_t *)(w + o_cbase), (uint32_t *)(w + o_entry), (uint32_t *)(w + o_sexit),
                     (uint32_t *)(w + o_bits), (uint32_t *)(w + o_cnt),   (uint64_t *)(w + o_cout),  (uint32_t *)(w + o_cflag),
                     (uint64_t *)(w + o_ctb),  (uint64_t *)(w + o_cob),   (JTok *)(w + o_tok),       tok_cap,
                     (JTok *)(w + o_ltok),     (uint32_t *)(w + o_maxd),  (uint32_t *)(w + o_ptr),   (uint32_t *)(w + o_pass),
                     jchunk(in_ext),           in_ext,                    out_ext};
    }
};

// the ptr array's first byte: out_off[0] less the continuation's history, rounded down to 16 bytes
EZ_HD uint64_t jg0(const DecompressArgs &A) { return (A.out_off[0] - (A.c_on ? A.c_hist : 0)) & ~15ull; }

// JWork.cflag: kJFBad, kJFReset and kJFResetLate (output before the MetaReset in its chunk) are KzSum.fl's
// bits; kJFOutFirst: a token before the MetaReset in its chunk
enum : uint32_t { kJFBad = kZBad, kJFReset = kZReset, kJFResetLate = kZResetLate, kJFOutFirst = 8 };

// the batch in global memory as an accessor: the 16 bytes at batch offset y, zeros past the batch
struct KjBatch {
    const uint8_t *in;
    uint64_t total;  // in_off[count]
    EZ_HD V16 operator()(uint64_t y) const { return y + 16 <= total ? ld16v(in + y) : ld_clamped(in + y, in, in + total); }
};

// ---- the chunk view: chunk c of the batch is bytes [c0, ce) of stream s, which starts at batch offset
// b0 and has nb bytes; live: the chunk exists and K2j still decodes its stream
struct KjChunk {
    uint32_t s;
    uint64_t b0;
    int32_t nb, c0, ce;
    bool live;
};
EZ_HD KjChunk kj_chunk(uint32_t c, const uint32_t *cbase, uint32_t count, const uint64_t *in_off, const JHead *head, int32_t jc) {
    KjChunk k;
    k.live = c < cbase[count];
    k.s = k.live ? last_le(cbase, count, c) : 0;
    k.live = k.live && !head[k.s].state;
    k.b0 = in_off[k.s];
    k.nb = (int32_t)(in_off[k.s + 1] - in_off[k.s]);
    k.c0 = (int32_t)(c - cbase[k.s]) * jc;
    k.ce = k.c0 + jc < k.nb ? k.c0 + jc : k.nb;
    return k;
}

// ---- the speculative walk of the chunk [c0, ce) of the stream at b0, with jadv_fast (ez_k2_parse.h: no
// checks): the warm-up from kj_warm0(c0) (nothing recorded), then the positions visited in the chunk
// into bm[0 .. kJW); returns where the walk leaves the chunk.  Reads at(y) for y in [b0 + warm0, b0 + ce).
// (K2z's kz_spec: a compile-time chunk, a warm-up of one chunk, padding clamped at the stream's end.)
EZ_HD int32_t kj_warm0(int32_t c0) { return c0 > kJWarm ? c0 - kJWarm : 0; }
template <class At>
EZ_HD int32_t kj_spec_walk(At at, uint64_t b0, int32_t c0, int32_t ce, uint32_t *bm) {
    for (int k = 0; k < kJW; k++) bm[k] = 0;
    int32_t p = kj_warm0(c0);
    while (p < c0) p += jadv_fast(at(b0 + (uint64_t)p));
    while (p < ce) {
        bm[(p - c0) >> 5] |= 1u << ((p - c0) & 31);
        p += jadv_fast(at(b0 + (uint64_t)p));
    }
    return p;
}

// ---- the follow walk: the chunk's true exit for the entry a, the true chain's position at or past c0.
// An entry at or past the chunk's end (inside a long token) passes through; else the chain from a
// until a position the speculative walk recorded in bits (the rest of the chain is then the
// speculative one: its exit *sexit is the true exit) or the chunk's end.  Chunk 0's entry 0 is its
// speculative walk's first position.  (K2z's kz_verify, without the padding clamp.)
template <class At>
EZ_HD int32_t kj_follow(At at, uint64_t b0, int32_t a, int32_t c0, int32_t ce, const uint32_t *bits, const uint32_t *sexit) {
    if (a >= ce) return a;
    int32_t q = a < c0 ? c0 : a;  // (a < c0 cannot happen: a speculative exit is >= its chunk's end)
    while (q < ce) {
        if ((bits[(q - c0) >> 5] >> ((q - c0) & 31)) & 1u) return (int32_t)*sexit;
        q += jadv_fast(at(b0 + (uint64_t)q));
    }
    return q;
}

// kj_fix: the chunk that holds the true entry e of chunk jf (its predecessor's true exit): jf itself,
// or a later one when e lies past chunk jf (inside a long token: no token starts in the chunks it
// covers), nch when e is at or past the stream's end
EZ_HD uint32_t kj_holder(int32_t e, uint32_t jf, int32_t nb, uint32_t nch, int32_t jc) {
    if (e >= nb) return nch;
    return e >= (int32_t)(jf + 1) * jc ? (uint32_t)(e / jc) : jf;
}
// the chain must end exactly at the stream's end (else the last token runs past the input; a
// Reader's read-ahead, c_on, stops before that token: kj_tok finds it)
EZ_HD bool kj_chain_bad(int32_t last, int32_t nb, bool c_on) { return c_on ? last < nb : last != nb; }

// ---- the token walk: the true chain of the chunk ending at ce from its entry, every form checked by
// k2_scan; a record per token into rec[0 .. kJRec) (output positions from the chunk's start).  In a
// continuation (partial) the step the input ends inside of stops the chain and is written to H
// (one chunk of the stream meets it).  brk(out): a Break meta at the chunk's output position out, called
// only with want_breaks (one-stream batches).
// (K2z's kz_sum with records, the continuation's stop and Breaks; no padding clamp and no exit check.)
struct KjSum {
    uint32_t n;     // token records
    uint32_t fl;    // kJF* bits, bits 8-15: the chunk's last MetaReset
    uint32_t maxd;  // the longest copy distance
    uint64_t out;   // output bytes
};
template <class At, class Brk>
EZ_HD KjSum kj_tok_walk(At at, uint64_t b0, int32_t nb, int32_t ce, int32_t entry, int32_t lim32, int64_t limit, bool partial, JTok *rec,
                        JHead &H, bool want_breaks, Brk brk) {
    KjSum r{0, 0, 0, 0};
    int32_t p = entry;
    while (p < ce) {
        K2Tok t;
        const V16 h = at(b0 + (uint64_t)p);
        const int k = k2_scan(h, p, nb, lim32, limit, t, partial);
        if (k == kParseHandOver || (k == kParseToken && r.n >= kJRec)) {
            r.fl |= kJFBad;
            break;
        }
        if (k == kScanTail) {
            H.tstop = p;
            H.tj = t.adv ? t.j : 0;
            H.tL = t.adv ? t.L : 0;
            break;
        }
        if (k == kScanReset) {
            r.fl |= (r.out ? kJFResetLate : 0) | kJFReset | (r.n == 0 ? 0 : kJFOutFirst);
            r.fl = (r.fl & 0xffu) | (t.marg << 8);
        } else if (k == kParseToken) {
            rec[r.n++] = JTok{(uint32_t)r.out, (uint32_t)t.L, t.cp ? (kJCopy | t.D) : 0u, (uint32_t)(p + t.j)};
            r.maxd = t.cp && t.D > r.maxd ? t.D : r.maxd;
            r.out += (uint64_t)t.L;
        } else if (k == kParseSkip && want_breaks) {
            if (((uint32_t)h.lo & 0xffffu) == (0x80u | ((kMetaBreak | kMetaLen0) << 8))) brk(r.out);
        }
        p += t.adv;
    }
    return r;
}

// ---- kj_scan's checks.  Per chunk, with the stream's output before it: a MetaReset only before any
// output (kz_reset_bad), any token (K2j's own flag: the scan's obefore counts output bytes) and, in a
// continuation, any output of the Reader's stream before this input (pos0)
EZ_HD bool kj_chunk_bad(uint32_t fl, uint64_t obefore, bool pos0) {
    return (fl & kJFBad) || kz_reset_bad(fl, obefore) || ((fl & kJFReset) && ((fl & kJFOutFirst) || pos0));
}
// (c_on) the bytes of a literal at the input's end whose body runs past it: they are output too
EZ_HD uint64_t kj_tail(bool c_on, const JHead &H, int32_t nb) {
    if (!c_on || H.tj <= 0) return 0;
    const int64_t left = (int64_t)(nb - H.tstop - H.tj);
    return (uint64_t)(H.tL < left ? H.tL : left);
}
// On the scanned totals of a stream no chunk of which is bad: kz_end_ok's window checks ("missed meta",
// a token or a continuation's literal header before the window is set; ErrOverflow, a distance past the
// window, is the exact decoder's to report) -- the chain's end is kj_fix's check, kj_chain_bad -- and
// the slot of cap bytes, which K2z does not have: nospace (the caller's end_state[0] = -2).
EZ_HD bool kj_stream_bad(uint64_t total, int32_t bsl, uint32_t maxd, uint64_t cap, bool c_on, const JHead &H, int32_t nb, bool &nospace) {
    nospace = false;
    if (!kz_end_ok(0, 0, total | (uint64_t)(c_on && H.tj > 0), bsl, maxd)) return true;
    nospace = total + kj_tail(c_on, H, nb) > cap;
    return nospace;
}

// ---- output bytes [q, q + n) of stream s (n <= 16, inside its output): bytes into by, pointers into pt.
// Pointers and the ptr array count from g0 = out_off[0] rounded down to 16 bytes: a batch may be a view
// into a larger one (absolute offsets), whose bytes before out_off[0] are never touched.
EZ_HD void kj_piece(const DecompressArgs &A, const JWork &W, const JHead &H, uint32_t s, uint64_t q, uint32_t n, uint64_t g0, uint32_t *by,
                    uint32_t *pt) {
    const uint64_t base = A.out_off[s];
    const uint32_t hb = A.c_on ? (uint32_t)A.c_hist : 0u;  // history bytes before the output (a copy may read them)
    const uint32_t p0 = (uint32_t)(q - base);
    // the token holding p0: the last record with dst <= p0; the next ones by walking on
    const JTok *tk = W.tok + H.tok0;
    uint64_t a = last_le_by(H.ntok, [&](uint64_t m) { return tk[m].dst; }, p0);
    JTok t = tk[a];
    uint32_t nxt = a + 1 < H.ntok ? tk[a + 1].dst : 0xffffffffu;
    const uint8_t *in = A.in + A.in_off[s];
    if (n == 16 && p0 + 16 <= t.dst + t.L) {  // the 16 bytes inside one token (long literals, runs, zeros)
        const uint32_t x = (uint32_t)(base + p0 - g0);
        if (t.kd == 0) {
            const V16 v = KjBatch{A.in, A.in_off[A.count]}(A.in_off[s] + t.src + (p0 - t.dst));
            by[0] = (uint32_t)v.lo, by[1] = (uint32_t)(v.lo >> 32), by[2] = (uint32_t)v.hi, by[3] = (uint32_t)(v.hi >> 32);
            for (uint32_t k = 0; k < 16; k++) pt[k] = x + k;
        } else if (t.kd == kJCopy) {
            for (uint32_t k = 0; k < 16; k++) pt[k] = x + k;
        } else {
            const uint32_t D = t.kd & ~kJCopy;
            for (uint32_t k = 0; k < 16; k++) pt[k] = p0 + k + hb >= D ? x + k - D : kJZero;
        }
        return;
    }
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t p = p0 + k;
        while (p >= nxt) {
            a++;
            t = tk[a];
            nxt = a + 1 < H.ntok ? tk[a + 1].dst : 0xffffffffu;
        }
        const uint32_t x = (uint32_t)(base + p - g0);
        uint32_t v = 0;
        if (t.kd == 0) {  // literal
            v = in[t.src + (p - t.dst)];
            pt[k] = x;
        } else if (t.kd == kJCopy) {  // zero region
            pt[k] = x;
        } else {
            const uint32_t D = t.kd & ~kJCopy;
            pt[k] = p + hb >= D ? x - D : kJZero;
        }
        by[k >> 2] |= v << (8 * (k & 3));
    }
}

}  // namespace ez
