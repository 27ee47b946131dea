// Host check of the parse primitives the batch decoders share (eazy_amd/csrc/ez_k2_parse.h): the same
// source, compiled for the CPU, compared header by header with the oracle's Decoder
// (oracle/eazy_oracle.c: or_dec_tag, or_dec_offset, or_dec_meta) and with the steps readTag /
// continueMetaTag (reader.go:218-325) take on them.
//   k2_parse_check            prints the count of every class, exits 1 at the first mismatch
//
// Over 16-byte headers h (every value of bytes 0..2; edge values in bytes 3..7; zero runs of 1..16;
// the header metas):
//  - step:    jadv_fast(h) >= 1, and == k2_scan's adv unless k2_scan hands the form over
//  - common:  fast_tok(h.lo) >= 0  =>  its L, adv, D, cp are k2_scan's
//  - oracle:  a kParseToken's L, j, D, adv are the Decoder's; padding, Break, Ver 0, Magic and Reset
//             advance as readTag does; what the Reader rejects k2_scan hands over; what the Reader
//             accepts k2_scan hands over only for the documented forms (a wide meta length, a
//             distance or 4-byte length of 2^30 or more, a literal past the input)
//  - partial: with the input cut at every nb inside the header (the bytes past it zero, as past a
//             one-stream batch): kScanTail with adv == 0 exactly where readTag returns ErrShortBuffer,
//             for every form the Reader accepts; a literal whose header is whole and whose body is
//             not: kScanTail with its j and L.  (A form the Reader rejects may stop at a tail or be
//             handed over: the host Reader resumes at that token and reports its error.)
// (of the common header this check uses rnd() and the count printer only)
#include "k2_check_common.h"

using k2check::rnd;

namespace {

constexpr int32_t kNb = 1 << 30;
constexpr int32_t kNoLim = 0x7fffffff;
// the oracle's input length for a whole header: the input ends far away (a meta's length may be
// anything; the Decoder reads the header's bytes only, at most 11)
constexpr int64_t kFar = 1ll << 40;

enum { R_SHORT, R_ERR, R_LIT, R_COPY, R_SKIP, R_RESET };
struct Ref {
    int kind;
    int64_t L, j, D, adv, marg;
};

// readTag at position 0 of b[0, n) (b[0] != 0), a fresh Reader with no limit and no options
Ref ref_step(const uint8_t *b, int64_t n) {
    Ref r{};
    int tag;
    int64_t l, i;
    int e = or_dec_tag(b, n, 0, &tag, &l, &i);
    if (e) {
        r.kind = e == OR_ESHORTBUF ? R_SHORT : R_ERR;
        return r;
    }
    if (tag == 0x80 && l == 0) {  // continueMetaTag
        int64_t meta, ml, k;
        e = or_dec_meta(b, n, i, &meta, &ml, &k);
        if (e) {
            r.kind = e == OR_ESHORTBUF ? R_SHORT : R_ERR;
            return r;
        }
        if (k + ml > n) {
            r.kind = R_SHORT;
            return r;
        }
        static const int64_t tag_len[4] = {4, 1, 1, 0};
        const int64_t ty = meta >> 3;
        r.kind = R_ERR;
        if (ty >= 4 || ml != tag_len[ty]) return r;
        if (ty == 0 && memcmp(b + k, "eazy", 4) != 0) return r;
        if (ty == 1 && b[k] > 0) return r;
        if (ty == 2 && b[k] > 32) return r;
        r.kind = ty == 2 ? R_RESET : R_SKIP;
        r.marg = ty == 2 ? b[k] : 0;
        r.adv = k + ml;
        return r;
    }
    r.L = l;
    if (tag == 0) {
        r.kind = R_LIT;
        r.j = i;
        r.adv = i + l;
        return r;
    }
    int64_t off, k;
    e = or_dec_offset(b, n, i, l, &off, &k);
    if (e) {
        r.kind = e == OR_ESHORTBUF ? R_SHORT : R_ERR;
        return r;
    }
    r.kind = R_COPY;
    r.D = off;
    r.adv = k;
    return r;
}

ez::V16 v16(const uint8_t *h) {
    ez::V16 v;
    memcpy(&v.lo, h, 8);
    memcpy(&v.hi, h + 8, 8);
    return v;
}

struct Counts {
    uint64_t headers, pad, skip, reset, lit, copy, zero_region, rejected, handed_wide_meta, handed_big, fast, part_cuts, tail_header,
        tail_literal, tail_rejected, part_token, part_pad;
    uint64_t m_break, m_reset_ok, m_reset_bad, m_ver_ok, m_ver_bad, m_magic_ok, m_magic_bad, m_wide, m_unknown;
} C;

[[noreturn]] void fail(const char *what, const uint8_t *h, int nb, int r, const ez::K2Tok &t, const Ref &o, int32_t jf) {
    std::printf("MISMATCH %s: header", what);
    for (int k = 0; k < 16; k++) std::printf(" %02x", h[k]);
    std::printf(" nb %d | k2_scan r %d adv %d L %d j %d D %u cp %d marg %u | jadv_fast %d | oracle kind %d adv %lld L %lld j %lld D %lld marg %lld\n",
                nb, r, t.adv, t.L, t.j, t.D, (int)t.cp, t.marg, jf, o.kind, (long long)o.adv, (long long)o.L, (long long)o.j,
                (long long)o.D, (long long)o.marg);
    std::exit(1);
}

int zero_run(const uint8_t *h) {
    int k = 0;
    while (k < 16 && h[k] == 0) k++;
    return k;
}

void meta_class(const uint8_t *h, const Ref &o) {
    const uint32_t mt = h[1] & 0xf8, ml = h[1] & 7;
    if (ml == 6) C.m_wide++;
    else if (mt == 0x18 && o.kind == R_SKIP) C.m_break++;
    else if (mt == 0x10 && ml == 0) (o.kind == R_RESET ? C.m_reset_ok : C.m_reset_bad)++;
    else if (mt == 0x08 && ml == 0) (o.kind == R_SKIP ? C.m_ver_ok : C.m_ver_bad)++;
    else if (mt == 0x00 && ml == 2) (o.kind == R_SKIP ? C.m_magic_ok : C.m_magic_bad)++;
    else if (mt >= 0x20) C.m_unknown++;
}

// the whole header: the input does not end near it
void check_full(const uint8_t *h) {
    C.headers++;
    const ez::V16 v = v16(h);
    ez::K2Tok t;
    const int r = ez::k2_scan(v, 0, kNb, kNoLim, 0, t);
    const int32_t jf = ez::jadv_fast(v);
    Ref o{};
    if (jf < 1) fail("jadv_fast < 1", h, kNb, r, t, o, jf);
    if (r != ez::kParseHandOver && jf != t.adv) fail("jadv_fast != k2_scan adv", h, kNb, r, t, o, jf);
    int32_t fL, fadv;
    uint32_t fD;
    bool fcp;
    if (ez::fast_tok(v.lo, fL, fadv, fD, fcp) >= 0) {
        C.fast++;
        if (r != ez::kParseToken || fL != t.L || fadv != t.adv || fcp != t.cp || (fcp && fD != t.D)) {
            std::printf("fast_tok: L %d adv %d D %u cp %d\n", fL, fadv, fD, (int)fcp);
            fail("fast_tok != k2_scan", h, kNb, r, t, o, jf);
        }
    }
    if (h[0] == 0) {  // padding: readTag skips the zeros (a step takes at most 16)
        C.pad++;
        if (r != ez::kParseSkip || t.adv != zero_run(h)) fail("padding", h, kNb, r, t, o, jf);
        return;
    }
    o = ref_step(h, kFar);
    if (h[0] == 0x80) meta_class(h, o);
    switch (o.kind) {
    case R_SHORT:
        fail("oracle short on 16 bytes", h, kNb, r, t, o, jf);
    case R_ERR:
        C.rejected++;
        if (r != ez::kParseHandOver) fail("rejected form not handed over", h, kNb, r, t, o, jf);
        return;
    case R_SKIP:
    case R_RESET:
        if (r == ez::kParseHandOver && (h[1] & 7) == 6) {
            C.handed_wide_meta++;
            return;
        }
        if (r != (o.kind == R_RESET ? ez::kScanReset : ez::kParseSkip) || t.adv != o.adv || (o.kind == R_RESET && t.marg != o.marg))
            fail("meta", h, kNb, r, t, o, jf);
        (o.kind == R_RESET ? C.reset : C.skip)++;
        return;
    case R_LIT:
        if (r == ez::kParseHandOver && o.adv > kNb) {
            C.handed_big++;
            return;
        }
        if (r != ez::kParseToken || t.cp || t.L != o.L || t.j != o.j || t.adv != o.adv || t.D != 0) fail("literal", h, kNb, r, t, o, jf);
        C.lit++;
        return;
    case R_COPY:
        if (r == ez::kParseHandOver && (o.D >= (1ll << 30) || o.L >= (1ll << 30) + 65916)) {
            C.handed_big++;
            return;
        }
        if (r != ez::kParseToken || !t.cp || t.L != o.L || t.D != o.D || t.adv != o.adv) fail("copy", h, kNb, r, t, o, jf);
        C.copy++;
        if (o.D == 0) C.zero_region++;
        return;
    }
}

// the input cut at nb = 1..16 (partial = true, the bytes past the cut zero)
void check_partial(const uint8_t *h) {
    for (int nb = 1; nb <= 16; nb++) {
        uint8_t z[16] = {0};
        memcpy(z, h, nb);
        C.part_cuts++;
        const ez::V16 v = v16(z);
        ez::K2Tok t;
        const int r = ez::k2_scan(v, 0, nb, kNoLim, 0, t, true);
        Ref o{};
        if (z[0] == 0) {
            const int run = zero_run(z) < nb ? zero_run(z) : nb;
            if (r != ez::kParseSkip || t.adv != run) fail("partial padding", z, nb, r, t, o, 0);
            C.part_pad++;
            continue;
        }
        o = ref_step(z, nb);
        const Ref whole = ref_step(z, kFar);  // the form with the unseen bytes zero: rejected whatever follows?
        const bool tail0 = r == ez::kScanTail && t.adv == 0;
        const bool wide = z[0] == 0x80 && (z[1] & 7) == 6;
        switch (o.kind) {
        case R_SHORT:
            if (whole.kind != R_ERR && !wide) {
                if (!tail0) fail("partial: header short, no tail", z, nb, r, t, o, 0);
                C.tail_header++;
            } else {
                if (!tail0 && r != ez::kParseHandOver) fail("partial: rejected form goes on", z, nb, r, t, o, 0);
                C.tail_rejected++;
            }
            break;
        case R_ERR:
            if (!tail0 && r != ez::kParseHandOver) fail("partial: rejected form goes on", z, nb, r, t, o, 0);
            C.tail_rejected++;
            break;
        case R_SKIP:
        case R_RESET:
            if (wide && r == ez::kParseHandOver) break;
            if (r != (o.kind == R_RESET ? ez::kScanReset : ez::kParseSkip) || t.adv != o.adv) fail("partial meta", z, nb, r, t, o, 0);
            C.part_token++;
            break;
        case R_LIT:
            if (r == ez::kParseHandOver && o.L >= (1ll << 30) + 65916) break;
            if (o.adv > nb) {  // the header whole, the body not
                if (r != ez::kScanTail || t.adv != o.adv || t.j != o.j || t.L != o.L) fail("partial: literal tail", z, nb, r, t, o, 0);
                C.tail_literal++;
            } else {
                if (r != ez::kParseToken || t.cp || t.L != o.L || t.j != o.j || t.adv != o.adv) fail("partial literal", z, nb, r, t, o, 0);
                C.part_token++;
            }
            break;
        case R_COPY:
            if (r == ez::kParseHandOver && (o.D >= (1ll << 30) || o.L >= (1ll << 30) + 65916)) break;
            if (r != ez::kParseToken || !t.cp || t.L != o.L || t.D != o.D || t.adv != o.adv) fail("partial copy", z, nb, r, t, o, 0);
            C.part_token++;
            break;
        }
    }
}

void fill(uint8_t *h, int from) {
    const uint64_t a = rnd(), b = rnd();
    for (int k = from; k < 16; k++) h[k] = (uint8_t)((k < 8 ? a : b) >> (8 * (k & 7)));
}

const uint8_t kEdge[12] = {0x00, 0x7b, 0x7c, 0x7d, 0x7e, 0x7f, 0x80, 0xfb, 0xfc, 0xfd, 0xfe, 0xff};

}  // namespace

int main() {
    uint8_t h[16];
    // every value of bytes 0..2, the rest from the generator (one in 64 also cut at every nb)
    for (uint32_t x = 0; x < (1u << 24); x++) {
        h[0] = (uint8_t)x, h[1] = (uint8_t)(x >> 8), h[2] = (uint8_t)(x >> 16);
        fill(h, 3);
        check_full(h);
        if ((x * 2654435761u >> 26) == 0) check_partial(h);
    }
    // edge values in each of bytes 3..7, under every tag and edge values in bytes 1..2
    for (uint32_t b0 = 0; b0 < 256; b0++)
        for (int e1 = 0; e1 < 14; e1++)
            for (int e2 = 0; e2 < 14; e2++)
                for (int p = 3; p <= 7; p++)
                    for (int e = 0; e < 12; e++) {
                        fill(h, 1);
                        h[0] = (uint8_t)b0;
                        if (e1 < 12) h[1] = kEdge[e1];
                        if (e2 < 12) h[2] = kEdge[e2];
                        h[p] = kEdge[e];
                        if (e & 1)  // (and an edge value next to it: the 4-byte lengths and offsets of 2^30)
                            h[p == 7 ? 3 : p + 1] = kEdge[(e1 + e2 + p) % 12];
                        check_full(h);
                        if (e1 >= 10 || e2 >= 10 || p == 3) check_partial(h);
                    }
    // zero runs of 1..16 (a run of 16 is all there is)
    for (int run = 1; run <= 16; run++)
        for (int k = 0; k < 4096; k++) {
            fill(h, 0);
            memset(h, 0, run);
            if (run < 16 && h[run] == 0) h[run] = 0x41;
            check_full(h);
            check_partial(h);
        }
    // the metas: Break, Reset 0..33, Ver 0 and 1, Magic right and wrong, wide lengths, unknown types
    for (int k = 0; k < 64; k++) {
        auto meta = [&](uint8_t m, const char *arg, int n) {
            fill(h, 0);
            h[0] = 0x80, h[1] = m;
            memcpy(h + 2, arg, n);
            check_full(h);
            check_partial(h);
        };
        meta(0x18 | 7, "", 0);
        for (int a = 0; a <= 33; a++) {
            const char c = (char)a;
            meta(0x10, &c, 1);
            meta(0x10 | 6, "\x01", 1);  // Reset with a wide length of 1: the Reader takes it, k2_scan hands it over
        }
        meta(0x08, "\x00", 1);
        meta(0x08, "\x01", 1);
        meta(0x02, "eazy", 4);
        meta(0x02, "eazx", 4);
        meta(0x02, "Eazy", 4);
        meta(0x00 | 6, "\x04" "eazy", 5);
        meta(0x18 | 6, "\x00", 1);
        meta(0x08 | 6, "\xfc\x01", 2);
        for (int ty = 4; ty < 32; ty++) meta((uint8_t)(ty << 3 | (k & 7)), "", 0);
    }
#define P(f) K2_COUNT(C, 18, f)
    P(headers); P(pad); P(skip); P(reset); P(lit); P(copy); P(zero_region); P(rejected); P(handed_wide_meta); P(handed_big); P(fast);
    P(part_cuts); P(part_pad); P(part_token); P(tail_header); P(tail_literal); P(tail_rejected);
    P(m_break); P(m_reset_ok); P(m_reset_bad); P(m_ver_ok); P(m_ver_bad); P(m_magic_ok); P(m_magic_bad); P(m_wide); P(m_unknown);
    std::printf("ok\n");
    return 0;
}
