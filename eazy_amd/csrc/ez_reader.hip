// ez_reader.hip — the Reader handle of include/eazy.h: the Read-by-Read decode through two device
// buffers, and the two read-ahead paths (a whole stream decoded at the first Read; the buffered input
// of an io.Reader decoded at once) whose Reads are served through a pinned staging window.
#include <hip/hip_runtime.h>

#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <vector>

#include "ez_format.h"
#include "ez_host.h"
#include "ez_internal.h"

using namespace ez;

struct ez_reader {
    int device = 0;
    ez::DecodeState st{};
    int64_t limit = 0;
    int require_magic = 0, skip_meta = 0;
    DBuf in, obuf[2], dstate, meta;  // obuf: history + output, double-buffered (ez_reader_read)
    int cur = 0;
    hipStream_t stream = nullptr;
    // whole-stream decode (ez_reader_set_whole): the stream decoded once by the batch path into a_out
    // (device memory), the Reads served from it through a pinned staging window
    int whole = 0;             // the caller's b is the whole stream (NewReaderBytes / ResetBytes)
    int tried = 0;             // tried since the last reset
    int ahead_on = 0;          // Reads are served from a_out[a_at .. a_n)
    uint64_t w_slot = 0;       // the slot the last whole-stream attempt decoded into (ez_reader_whole_slot)
    int w_launches = 0;        // the decode launches it made (ez_reader_whole_launches)
    DBuf a_in, a_out, a_meta, a_ws, a_brk, a_qws;  // kept across resets (grown, never shrunk); a_qws: the size query's scratch
    uint64_t a_n = 0, a_at = 0;             // bytes decoded; bytes served
    size_t a_blen = 0;                      // the input decoded (len(r.b) at the first Read)
    std::vector<uint64_t> brk;              // the Break metas' output positions, ascending
    size_t brk_next = 0;                    // the next one a Read has not reported
    int64_t end_bs = 0, end_pos = 0;        // the Reader's len(r.block) and r.pos after the stream
    uint8_t *stage = nullptr;               // pinned: srv[stage_at .. stage_at + stage_n)
    uint64_t stage_at = 0, stage_n = 0;
    const uint8_t *srv = nullptr;           // the device bytes the Reads are served from (a_out, or a read-ahead's)
    // read-ahead of a NewReader(io.Reader) handle (whole == 0, ez_reader_read): all the input buffered
    // at a Read decoded at once; its Reads are then served from srv[a_at .. a_n) (ahead_on stays 0)
    int s_on = 0;
    int64_t s_iend = 0;                     // the absolute input position the read-ahead consumed to
    int64_t s_skip = -1;                    // a read-ahead handed over at this absolute buffer end: none until more input
    int64_t s_count = 0;                    // read-aheads made (ez_reader_ahead_count)
    DBuf s_meta, s_ws;
};

extern "C" int ez_reader_new(int device, ez_reader **out) {
    *out = nullptr;
    DeviceGuard g(device);
    if (!g.ok) return EZ_EDEVICE;
    ez_reader *r = new ez_reader();
    r->device = device;
    if (hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking) != hipSuccess) {
        delete r;
        return EZ_EDEVICE;
    }
    if (r->dstate.ensure(sizeof(ez::DecodeState)) || r->meta.ensure(64)) {
        ez_reader_free(r);
        return EZ_EDEVICE;
    }
    *out = r;
    return EZ_OK;
}

extern "C" void ez_reader_free(ez_reader *r) {
    if (!r) return;
    DeviceGuard g(r->device);
    for (DBuf *b : {&r->in, &r->obuf[0], &r->obuf[1], &r->dstate, &r->meta, &r->a_in, &r->a_out, &r->a_meta, &r->a_ws, &r->a_brk, &r->a_qws,
                    &r->s_meta, &r->s_ws})
        b->release();
    if (r->stage) (void)hipHostFree(r->stage);
    if (r->stream) (void)hipStreamDestroy(r->stream);
    delete r;
}

extern "C" int ez_reader_configure(ez_reader *r, int64_t block_size_limit, int require_magic, int skip_meta) {
    r->limit = block_size_limit;
    r->require_magic = require_magic ? 1 : 0;
    r->skip_meta = skip_meta ? 1 : 0;
    return EZ_OK;
}

// ResetBytes reader.go:102-113: block = block[:0], pos = 0, state = 0
// (r.d.Ver is kept, as in the reference).
extern "C" int ez_reader_reset(ez_reader *r) {
    const int32_t ver = r->st.ver;
    r->st = ez::DecodeState{};
    r->st.ver = ver;
    r->tried = 0;
    r->ahead_on = 0;
    r->s_on = 0;
    r->s_skip = -1;
    r->a_n = r->a_at = 0;
    r->brk.clear();
    r->brk_next = 0;
    r->stage_n = 0;
    return EZ_OK;
}

extern "C" int ez_reader_set_whole(ez_reader *r, int whole) {
    r->whole = whole ? 1 : 0;
    return EZ_OK;
}

extern "C" int ez_reader_whole_decoded(const ez_reader *r) { return r->ahead_on; }

extern "C" uint64_t ez_reader_whole_slot(const ez_reader *r) { return r->w_slot; }

extern "C" int ez_reader_whole_launches(const ez_reader *r) { return r->w_launches; }

extern "C" int64_t ez_reader_ahead_count(const ez_reader *r) { return r->s_count; }

extern "C" int ez_reader_pending(const ez_reader *r) { return r->st.state != 0 ? 1 : 0; }

namespace {
// K2j's workspace for Reader handles, one per device: a whole-stream decode is synchronous, so the
// handles of a device take turns with it (a handle of its own would be allocated anew for every
// NewReaderBytes, tens of ms for a large stream)
struct ReaderJws {
    std::mutex mu;
    DBuf buf;
};
ReaderJws &reader_jws(int dev) {
    static std::mutex m;
    static std::map<int, ReaderJws *> all;
    std::lock_guard<std::mutex> lk(m);
    ReaderJws *&p = all[dev];
    if (!p) p = new ReaderJws();
    return *p;
}

// The handle's turn with its device's workspace, kept until the decode has been waited for; `need`
// bytes of it go into a (0: a decoder that takes none).  Not owned when they could not be had.
std::unique_lock<std::mutex> jws_lease(const ez_reader *r, ez::DecompressArgs &a, uint64_t need) {
    ReaderJws &J = reader_jws(r->device);
    std::unique_lock<std::mutex> lk(J.mu);
    if (need) {
        if (J.buf.ensure(need)) return std::unique_lock<std::mutex>();
        a.jws = J.buf.p;
        a.jws_cap = J.buf.cap;
    }
    return lk;
}

constexpr size_t kAheadMax = ((size_t)1 << 30) - 64;  // the largest output slot (K2t takes slots below 2^30)
constexpr size_t kAheadBrk = (size_t)1 << 16;         // Break positions recorded (more: Read by Read)
constexpr size_t kStage = (size_t)4 << 20;            // the pinned staging window (host memory per Reader)

// the pinned staging window, allocated at a handle's first read-ahead
bool stage_ready(ez_reader *r) {
    if (!r->stage && hipHostMalloc((void **)&r->stage, kStage, hipHostMallocDefault) != hipSuccess) r->stage = nullptr;
    return r->stage != nullptr;
}

// One stream's args on the handle: the input, the output buffer and the stream's meta block
// [in_off 2][out_off 2][out_size][status][end_state...] on the device
ez::DecompressArgs stream_args(const ez_reader *r, const DBuf &in, uint8_t *out, uint64_t *dm) {
    ez::DecompressArgs a{};
    a.in = in.as<uint8_t>();
    a.in_off = dm;
    a.out = out;
    a.out_off = dm + 2;
    a.count = 1;
    a.block_size_limit = r->limit;
    return a;
}

// ... of a read-ahead: a batch decode into a slot of cap bytes that reports the size, the status, the
// Reader's state at the end and the Break positions
ez::DecompressArgs ahead_args(const ez_reader *r, const DBuf &in, uint8_t *out, uint64_t *dm, const DBuf &ws, size_t cap) {
    ez::DecompressArgs a = stream_args(r, in, out, dm);
    a.out_size = dm + 4;
    a.status = (int32_t *)(dm + 5);
    a.end_state = (int64_t *)(dm + 6);
    a.breaks = r->a_brk.as<uint64_t>();
    a.breaks_cap = kAheadBrk;
    a.slow = ws.as<uint32_t>();
    a.max_out = cap;
    return a;
}

// The nbrk Break positions a read-ahead recorded, into r->brk: each moved by `shift`, ascending.  A
// failed copy leaves r->brk empty.  (Nothing reads brk while neither s_on nor ahead_on is set -- each of
// ez_reader_read's uses is under one of them -- and a handle that reads ahead has neither: stream_ahead
// runs with s_on clear on a handle that is not `whole`, reader_ahead with ahead_on clear on one that is.)
bool fetch_breaks(ez_reader *r, uint64_t nbrk, uint64_t shift) {
    try {
        r->brk.resize((size_t)nbrk);
    } catch (...) {
        return false;
    }
    if (nbrk && hipMemcpy(r->brk.data(), r->a_brk.as<uint64_t>() + 1, 8 * nbrk, hipMemcpyDeviceToHost) != hipSuccess) {
        r->brk.clear();
        return false;
    }
    for (auto &x : r->brk) x += shift;
    std::sort(r->brk.begin(), r->brk.end());
    return true;
}

// The current decode buffer grown to `need` bytes, the history (its first H bytes) kept at its head
int grow_keep_history(ez_reader *r, size_t H, size_t need) {
    DBuf &cur = r->obuf[r->cur];
    if (cur.cap >= need) return EZ_OK;
    DBuf nb;
    if (nb.ensure(need)) return EZ_EDEVICE;
    if (H) EZ_HIP(hipMemcpyAsync(nb.p, cur.p, H, hipMemcpyDeviceToDevice, r->stream));
    EZ_HIP(hipStreamSynchronize(r->stream));
    cur.release();
    cur = nb;
    return EZ_OK;
}

// The next decode's history: the H2 device bytes that end at `end` to the head of the decode buffer
// `to`, which grows as needed -- with `drain`, once the work queued on the other buffer is done.
// The copy is queued; the caller waits for it, and flips r->cur where `to` is the other buffer.
int hand_history(ez_reader *r, DBuf &to, const uint8_t *end, size_t H2, bool drain) {
    if (to.cap < H2 + 16) {
        if (drain) EZ_HIP(hipStreamSynchronize(r->stream));
        if (to.ensure(H2 + 16)) return EZ_EDEVICE;
    }
    if (H2) EZ_HIP(hipMemcpyAsync(to.p, end - H2, H2, hipMemcpyDeviceToDevice, r->stream));
    return EZ_OK;
}

// Whole-stream decode (NewReaderBytes then Read to the end, the reference's common use): the batch
// path decodes b as one stream -- K2j, or K2t for a short one -- into a device slot, and the Reads are
// then served from that output.  The slot is exact: after the upload the decoded-size query (K2z, the
// parts route for a long stream) runs on the handle's stream, and its size and status come back with
// the meta block.  A stream the query gives an error, or one that decodes to more than 1 GiB, is left
// to Read-by-Read decoding at once, with no output buffer allocated; any other is decoded once.  (The
// decode cannot find that slot too small; if it reports so all the same, the stream is left to Read by
// Read as well: the slot does not grow.)  The decoders record every Break meta's output position, so
// the Reads stop at each with ErrBreak as Read by Read does (reader.go:312-313), and the Reader's state
// at the end (len(r.block), r.pos), so that input a caller supplies after the stream (a Reader set after
// NewReaderBytes) continues Read by Read.  It applies where it gives exactly the bytes and errors of
// Read-by-Read decoding: a clean end of stream (status OK), RequireMagic and SkipUnsupportedMeta off;
// anything else leaves the handle as it was and the exact decoder runs Read by Read.  Device buffers are
// kept in the handle, host memory is the 4 MiB staging window.  Returns 1 when the Reads are now
// served from the decoded bytes.
int reader_ahead(ez_reader *r, const uint8_t *b, size_t b_len) {
    r->tried = 1;
    r->w_slot = 0;
    r->w_launches = 0;
    if (b_len == 0 || b_len > ((size_t)1 << 28) || r->require_magic || r->skip_meta) return 0;
    const size_t ws = ez_decompress_workspace(1);
    constexpr size_t o_meta = 64;  // [in_off 2][out_off 2][out_size][status][end_state 2]
    if (r->a_in.ensure(b_len + 64) || r->a_meta.ensure(o_meta * 2) || r->a_ws.ensure(ws) || r->a_brk.ensure(8 * (kAheadBrk + 1)))
        return 0;
    if (!stage_ready(r)) return 0;
    if (hipMemcpyAsync(r->a_in.p, b, b_len, hipMemcpyHostToDevice, r->stream) != hipSuccess) return 0;
    uint64_t m[8] = {0, (uint64_t)b_len, 0, 0, 0, (uint64_t)(uint32_t)-7, (uint64_t)-1, (uint64_t)-1};
    if (hipMemcpyAsync(r->a_meta.p, m, sizeof m, hipMemcpyHostToDevice, r->stream) != hipSuccess) return 0;
    {  // the stream's decoded size and status
        ez::DecompressArgs q{};
        uint64_t *dm = r->a_meta.as<uint64_t>();
        q.in = r->a_in.as<uint8_t>();
        q.in_off = dm;
        q.out_size = dm + 4;
        q.status = (int32_t *)(dm + 5);
        q.count = 1;
        q.block_size_limit = r->limit;
        q.slow = r->a_ws.as<uint32_t>();
        q.in_bytes = b_len;
        // (the parts route's scratch is the handle's: a cache entry per handle stream would be allocated
        // anew for every NewReaderBytes; without it the query takes the wave route)
        if (!r->a_qws.ensure(ez::size_parts_workspace_bytes(1, b_len))) {
            q.jws = r->a_qws.p;
            q.jws_cap = r->a_qws.cap;
        } else {
            q.in_bytes = 0;
        }
        if (ez::launch_decompress_size(q, b_len, r->stream) != hipSuccess) return 0;
        if (hipMemcpyAsync(m, r->a_meta.p, sizeof m, hipMemcpyDeviceToHost, r->stream) != hipSuccess) return 0;
        if (hipStreamSynchronize(r->stream) != hipSuccess) return 0;
    }
    if ((int32_t)(m[5] & 0xffffffffu) != EZ_OK || m[4] > kAheadMax) return 0;
    const size_t cap = m[4] < 16 ? 16 : (size_t)((m[4] + 15) & ~(uint64_t)15);  // (a fast decoder takes slots of 16 bytes or more)
    if (r->a_out.ensure(cap + 64)) return 0;
    r->w_slot = cap;
    m[3] = cap;
    m[4] = m[5] = 0;
    uint64_t nbrk = 0;
    if (hipMemcpyAsync(r->a_meta.p, m, sizeof m, hipMemcpyHostToDevice, r->stream) != hipSuccess) return 0;
    if (hipMemsetAsync(r->a_brk.p, 0, 8, r->stream) != hipSuccess) return 0;
    ez::DecompressArgs a = ahead_args(r, r->a_in, r->a_out.as<uint8_t>(), r->a_meta.as<uint64_t>(), r->a_ws, cap);
    // one stream: K2j (chip-wide) for a long one, else the token-parallel wave
    a.force = b_len >= ((size_t)16 << 10) ? 'j' : 't';
    {
        const auto lk = jws_lease(r, a, a.force == 'j' ? ez::jump_workspace_bytes(1, b_len, cap) : 0);
        if (!lk) return 0;
        r->w_launches++;
        if (ez::launch_decompress(a, r->stream) != hipSuccess) return 0;
        if (hipMemcpyAsync(m, r->a_meta.p, sizeof m, hipMemcpyDeviceToHost, r->stream) != hipSuccess) return 0;
        if (hipMemcpyAsync(&nbrk, r->a_brk.p, 8, hipMemcpyDeviceToHost, r->stream) != hipSuccess) return 0;
        if (hipStreamSynchronize(r->stream) != hipSuccess) return 0;
    }
    const int status = (int32_t)(m[5] & 0xffffffffu);
    if (status != EZ_OK || m[4] > cap || nbrk > kAheadBrk || (int64_t)m[6] < 0) return 0;
    if (!fetch_breaks(r, nbrk, 0)) return 0;
    r->brk_next = 0;
    r->a_n = m[4];
    r->a_at = 0;
    r->a_blen = b_len;
    r->end_bs = (int64_t)m[6];
    r->end_pos = (int64_t)m[7];
    r->stage_at = r->stage_n = 0;
    r->srv = r->a_out.as<uint8_t>();
    r->ahead_on = 1;
    return 1;
}

// n bytes of the decoded stream from a_at into p (staged; a copy larger than the window goes direct)
int ahead_copy(ez_reader *r, uint8_t *p, size_t n) {
    while (n) {
        if (r->a_at < r->stage_at || r->a_at >= r->stage_at + r->stage_n) {
            const uint64_t left = r->a_n - r->a_at;
            if (n >= kStage) {
                if (hipMemcpy(p, r->srv + r->a_at, n, hipMemcpyDeviceToHost) != hipSuccess) return EZ_EDEVICE;
                r->a_at += n;
                return EZ_OK;
            }
            r->stage_at = r->a_at;
            r->stage_n = left < kStage ? left : kStage;
            if (hipMemcpy(r->stage, r->srv + r->a_at, r->stage_n, hipMemcpyDeviceToHost) != hipSuccess) {
                r->stage_n = 0;
                return EZ_EDEVICE;
            }
        }
        const uint64_t in_stage = r->stage_at + r->stage_n - r->a_at;
        const size_t k = n < in_stage ? n : (size_t)in_stage;
        memcpy(p, r->stage + (r->a_at - r->stage_at), k);
        p += k;
        n -= k;
        r->a_at += k;
    }
    return EZ_OK;
}

// A Read served from the decoded bytes: up to the next Break (reader.go:312-313: Read returns the bytes
// before it with ErrBreak, and a Read that starts at it returns 0 bytes with ErrBreak) or their end.
// EZ_OK when p is full, EZ_EBREAK at a Break, EZ_ESHORTBUF when the bytes ran out first (*n set in all
// three; what that means for the input position is the caller's), EZ_EDEVICE with nothing set.
int ahead_serve(ez_reader *r, uint8_t *p, size_t p_len, size_t *n) {
    const bool at_brk = r->brk_next < r->brk.size();
    const uint64_t lim = at_brk ? r->brk[r->brk_next] : r->a_n;
    const uint64_t left = lim - r->a_at;
    const size_t m = p_len < left ? p_len : (size_t)left;
    if (m && ahead_copy(r, p, m) != EZ_OK) return EZ_EDEVICE;
    *n = m;
    if (m == p_len) return EZ_OK;
    if (!at_brk) return EZ_ESHORTBUF;
    r->brk_next++;
    return EZ_EBREAK;
}

constexpr size_t kStreamMin = (size_t)8 << 10;  // buffered input a read-ahead takes at least

// Read-ahead of a NewReader(io.Reader) handle (the README's usage, reader.go:79-86, 116-141, 516-543):
// at a Read with nothing decoded ahead, every whole token of the buffered input b[i..b_len) is decoded
// at once on the device -- K2j continuing the stream from the handle's state: the window's history at
// the head of the decode buffer, a pending literal's bytes put in front, the chain stopping before a
// token the buffer ends inside of, whose literal bytes there are are output too (reader.go:166-168) --
// and the Reads are served from that output until it runs out.  Then Read asks for more input exactly
// where Read by Read would (the whole tokens are consumed, the state is the same), so the io.Reader
// sees the same calls and the caller the same bytes, Breaks and errors.  A buffer K2j hands over (an
// error, a MetaReset after output, a distance past the window, ...) is decoded Read by Read until more
// input arrives.  Returns 1 when the Reads are now served from the read-ahead.
int stream_ahead(ez_reader *r, const uint8_t *b, size_t b_len, size_t i, int64_t boff) {
    ez::DecodeState &st = r->st;
    const int64_t bend = boff + (int64_t)b_len;
    if (r->require_magic || r->skip_meta || b_len < i + kStreamMin || b_len > ((size_t)1 << 28) || bend == r->s_skip) return 0;
    if (st.state == 'c' || st.ver != 0 || st.bs > ((int64_t)1 << 30)) return 0;  // (mid-copy: after a Read that filled p)
    const size_t H = (size_t)st.hist, nin = b_len - i;
    // a pending literal (r.state 'l'): its next bytes are the input's first
    const size_t k = st.state == 'l' ? (st.len < (int64_t)nin ? (size_t)st.len : nin) : 0;
    const size_t n2 = nin - k;  // the input K2j decodes (none when the literal takes it all)
    const size_t ws = ez_decompress_workspace(1);
    if (r->in.ensure(n2 + 64) || r->s_meta.ensure(256) || r->s_ws.ensure(ws) || r->a_brk.ensure(8 * (kAheadBrk + 1))) return 0;
    if (!stage_ready(r)) return 0;
    if (n2 && hipMemcpyAsync(r->in.p, b + i + k, n2, hipMemcpyHostToDevice, r->stream) != hipSuccess) return 0;
    size_t cap = n2 ? 8 * n2 + 4096 : 0;
    for (;;) {
        if (cap > kAheadMax) return 0;
        if (grow_keep_history(r, H, H + k + cap + 64)) return 0;
        uint8_t *o = r->obuf[r->cur].as<uint8_t>();
        if (k && hipMemcpyAsync(o + H, b + i, k, hipMemcpyHostToDevice, r->stream) != hipSuccess) return 0;
        // [in_off 2][out_off 2][out_size][status][end_state 5][slow count (u32)]
        uint64_t m[12] = {0, (uint64_t)n2, (uint64_t)(H + k), (uint64_t)(H + k + cap), 0, 0, 0, 0, 0, 0, 0, 0};
        uint64_t nbrk = 0;
        if (n2) {
            uint64_t *dm = r->s_meta.as<uint64_t>();
            if (hipMemcpyAsync(dm, m, sizeof m, hipMemcpyHostToDevice, r->stream) != hipSuccess) return 0;
            if (hipMemsetAsync(r->a_brk.p, 0, 8, r->stream) != hipSuccess) return 0;
            if (hipMemsetAsync(r->s_ws.p, 0, 4, r->stream) != hipSuccess) return 0;
            ez::DecompressArgs a = ahead_args(r, r->in, o, dm, r->s_ws, cap);
            a.in_bytes = n2;
            a.out_bytes = cap;
            a.c_on = 1;
            a.c_bsl = st.bs == 0 ? -1 : __builtin_ctzll((uint64_t)st.bs);
            a.c_hist = H + k;
            a.c_pos0 = st.pos + (int64_t)k;
            {
                const auto lk = jws_lease(r, a, ez::jump_workspace_bytes(1, n2, cap + H + k + 16));
                if (!lk) return 0;
                if (ez::launch_decompress_jump(a, r->stream) != hipSuccess) return 0;
                if (hipMemcpyAsync(m, dm, sizeof m, hipMemcpyDeviceToHost, r->stream) != hipSuccess) return 0;
                if (hipMemcpyAsync(&nbrk, r->a_brk.p, 8, hipMemcpyDeviceToHost, r->stream) != hipSuccess) return 0;
                uint32_t slow = 0;
                if (hipMemcpyAsync(&slow, r->s_ws.p, 4, hipMemcpyDeviceToHost, r->stream) != hipSuccess) return 0;
                if (hipStreamSynchronize(r->stream) != hipSuccess) return 0;
                if (slow) {
                    if ((int64_t)m[6] == -2 && cap < kAheadMax) {  // the slot was too small
                        cap = cap < kAheadMax / 4 ? 4 * cap : kAheadMax;
                        continue;
                    }
                    r->s_skip = bend;  // handed over: Read by Read until more input arrives
                    return 0;
                }
            }
            if (nbrk > kAheadBrk) {
                r->s_skip = bend;
                return 0;
            }
        }
        // the chain's stop and a literal the input ends inside of
        const int64_t total = n2 ? (int64_t)m[4] : 0;
        const int64_t stop = n2 ? (int64_t)m[8] : 0, tj = n2 ? (int64_t)m[9] : 0, tL = n2 ? (int64_t)m[10] : 0;
        int64_t tail = 0;
        if (tj > 0) {
            tail = (int64_t)n2 - stop - tj < tL ? (int64_t)n2 - stop - tj : tL;
            if (tail > 0 &&
                hipMemcpyAsync(o + H + k + total, r->in.as<uint8_t>() + stop + tj, (size_t)tail, hipMemcpyDeviceToDevice, r->stream) != hipSuccess)
                return 0;
        }
        // (positions in the served bytes: the pending literal's come first)
        if (!fetch_breaks(r, nbrk, k)) return 0;
        // the Reader's state after the last whole token (or inside the literal the input ends in)
        const int64_t out_n = (int64_t)k + total + tail;
        ez::DecodeState ns = st;
        if (n2) ns.bs = (int64_t)m[6];
        ns.pos = st.pos + out_n;
        if (n2 == 0) {  // the pending literal took the whole input
            ns.len = st.len - (int64_t)k;
            ns.state = ns.len == 0 ? 0 : 'l';
        } else if (tj > 0) {
            ns.state = 'l';
            ns.len = tL - tail;
        } else {
            ns.state = 0;
            ns.len = 0;
        }
        ns.hist = ns.bs == 0 ? 0 : (ns.pos < ns.bs ? ns.pos : ns.bs);
        // the next decode's history: the window's last hist bytes, at the head of the other buffer
        const size_t H2 = (size_t)ns.hist;
        if (H2 > H + (size_t)out_n) return 0;  // (cannot happen: the history is decoded output)
        if (hand_history(r, r->obuf[r->cur ^ 1], o + H + out_n, H2, true)) return 0;
        if (hipStreamSynchronize(r->stream) != hipSuccess) return 0;
        r->cur ^= 1;  // (the served bytes stay in this buffer; the next decode writes the other)
        st = ns;
        r->srv = o + H;
        r->a_n = (uint64_t)out_n;
        r->a_at = 0;
        r->brk_next = 0;
        r->stage_at = r->stage_n = 0;
        // (a meta's first byte alone at the input's end: the Reader consumes it before it misses the
        // second, reader.go:276-279, so a stream that ends there ends clean and the next input starts a token)
        const bool lone = n2 && tj == 0 && stop == (int64_t)n2 - 1 && b[b_len - 1] == ez::kMeta;
        r->s_iend = boff + (int64_t)(n2 == 0 || tj > 0 || lone ? b_len : i + k + (size_t)stop);
        r->s_on = 1;
        r->s_count++;
        return 1;
    }
}

// Input after the decoded stream (a Reader set after NewReaderBytes, so more() supplied more): the
// handle continues Read by Read from the Reader's state at the stream's end -- len(r.block), r.pos, no
// token pending, version 0 (the whole decode takes only those) -- with the window's history, the last
// min(r.pos, len(r.block)) decoded bytes, at the head of the decode buffer.
int ahead_leave(ez_reader *r) {
    ez::DecodeState st{};
    st.bs = r->end_bs;
    st.pos = r->end_pos;
    st.hist = st.bs == 0 ? 0 : (st.pos < st.bs ? st.pos : st.bs);
    const size_t H = (size_t)st.hist;
    if (H > r->a_n) return EZ_EDEVICE;  // (cannot happen: the history is decoded output)
    if (hand_history(r, r->obuf[r->cur], r->a_out.as<uint8_t>() + r->a_n, H, false)) return EZ_EDEVICE;
    if (hipStreamSynchronize(r->stream) != hipSuccess) return EZ_EDEVICE;
    r->st = st;
    r->ahead_on = 0;
    return EZ_OK;
}
}  // namespace

void ez::reader_release_cached(int dev) {
    ReaderJws &J = reader_jws(dev);
    if (J.mu.try_lock()) {
        J.buf.release();
        J.mu.unlock();
    }
}

bool ez::reader_fill_cached(int dev, int byte, uint64_t *bytes) {
    ReaderJws &J = reader_jws(dev);
    if (!J.mu.try_lock()) return true;
    const bool ok = !J.buf.p || byte < 0 || hipMemset(J.buf.p, byte, J.buf.cap) == hipSuccess;
    *bytes += J.buf.p ? J.buf.cap : 0;
    J.mu.unlock();
    return ok;
}

// Input is uploaded in windows from b[i] on, not the whole of b per call: a Read loop over one large
// NewReaderBytes buffer then moves each input byte to the device about once.  A window that ends inside
// a token makes the decoder stop there with EZ_ESHORTBUF and nothing of that token consumed
// (reader.go:218-270; DecompressArgs.more, for the one byte the Reader would consume, a meta's first),
// so the next window resumes at exactly that token; a token longer than the window
// with no progress doubles the window.  The decoded block history sits in front of the output in one of
// two device buffers; after a call the last min(pos, bs) bytes are copied once into the head of the
// other buffer, which the next call decodes into.
extern "C" int ez_reader_read(ez_reader *r, const uint8_t *b, size_t b_len, size_t i, int64_t boff, uint8_t *p,
                              size_t p_len, size_t *n, size_t *i_out, int64_t *detail) {
    *n = 0;
    *i_out = i;
    if (detail) *detail = 0;
    if (p_len == 0) return EZ_OK;  // Read(p) with len(p) == 0 returns at once (reader.go:119)
    DeviceGuard g(r->device);
    if (!g.ok) return EZ_EDEVICE;
    // a fresh handle over a whole stream: decode it once (reader_ahead), then serve every Read from it
    if (!r->ahead_on && r->whole && !r->tried && i == 0 && boff == 0 && r->st.bs == 0 && r->st.pos == 0 && r->st.state == 0)
        (void)reader_ahead(r, b, b_len);
    if (r->ahead_on && r->a_at == r->a_n && r->brk_next == r->brk.size() && (uint64_t)boff + b_len > r->a_blen) {
        // the stream is served and input follows it: Read by Read from the Reader's state at its end
        if (ahead_leave(r) != EZ_OK) return EZ_EDEVICE;
    }
    // NewReader(io.Reader): the buffered input decoded ahead, the Reads served from it
    if (!r->whole && !r->s_on) (void)stream_ahead(r, b, b_len, i, boff);
    if (r->s_on) {
        const int e = ahead_serve(r, p, p_len, n);
        if (e == EZ_EDEVICE) return e;
        *i_out = (size_t)(r->s_iend - boff);  // (only read back when this returns ErrShortBuffer)
        if (e == EZ_ESHORTBUF) r->s_on = 0;   // served: Read asks for more input where Read by Read would
        return e;
    }
    if (r->ahead_on) {
        const int e = ahead_serve(r, p, p_len, n);  // (the input position is reported when the output is done)
        if (e == EZ_ESHORTBUF) *i_out = b_len;      // the stream's end: Read asks for more input and gets EOF
        return e;
    }
    const size_t H = (size_t)r->st.hist;
    if (grow_keep_history(r, H, H + p_len + 16)) return EZ_EDEVICE;
    DBuf &cur = r->obuf[r->cur];
    if (r->meta.ensure(64)) return EZ_EDEVICE;
    size_t win = p_len * 2 + 64 < ((size_t)1 << 16) ? ((size_t)1 << 16) : p_len * 2 + 64;
    size_t at = i, got = 0;
    int err = EZ_OK;
    for (;;) {
        const size_t take = b_len - at < win ? b_len - at : win;
        if (r->in.ensure(take + 16)) return EZ_EDEVICE;
        if (take) EZ_HIP(hipMemcpyAsync(r->in.p, b + at, take, hipMemcpyHostToDevice, r->stream));
        r->st.i = 0;
        EZ_HIP(hipMemcpyAsync(r->dstate.p, &r->st, sizeof(r->st), hipMemcpyHostToDevice, r->stream));
        uint64_t m[4] = {0, (uint64_t)take, (uint64_t)(H + got), (uint64_t)(H + p_len)};
        EZ_HIP(hipMemcpyAsync(r->meta.p, m, sizeof(m), hipMemcpyHostToDevice, r->stream));
        // (out_size and status stay null: the handle's state carries what the decode made and its error)
        ez::DecompressArgs a = stream_args(r, r->in, cur.as<uint8_t>(), r->meta.as<uint64_t>());
        a.require_magic = r->require_magic;
        a.skip_unsupported_meta = r->skip_meta;
        a.handle = 1;
        a.more = take < b_len - at;   // the window ends before the input does
        a.boff = boff + (int64_t)at;  // absolute offset of the window's first byte
        a.st = r->dstate.as<ez::DecodeState>();
        EZ_HIP(ez::launch_decompress(a, r->stream));
        EZ_HIP(hipMemcpyAsync(&r->st, r->dstate.p, sizeof(r->st), hipMemcpyDeviceToHost, r->stream));
        EZ_HIP(hipStreamSynchronize(r->stream));
        err = r->st.err;
        const size_t used = (size_t)r->st.i, made = (size_t)r->st.n;
        at += used;
        got += made;
        // the window, not the input, ran short: go on with the next one
        if (err == EZ_ESHORTBUF && take < b_len - (at - used) && got < p_len) {
            if (used == 0 && made == 0) win *= 2;
            continue;
        }
        break;
    }
    const size_t H2 = (size_t)r->st.hist;
    if (got) EZ_HIP(hipMemcpyAsync(p, cur.as<uint8_t>() + H, got, hipMemcpyDeviceToHost, r->stream));
    if (H2) {  // the next call decodes into the other buffer, behind this block's last H2 bytes
        if (hand_history(r, r->obuf[r->cur ^ 1], cur.as<uint8_t>() + H + got, H2, true)) return EZ_EDEVICE;
        r->cur ^= 1;
    }
    EZ_HIP(hipStreamSynchronize(r->stream));
    *n = got;
    *i_out = at;
    if (detail) *detail = r->st.detail;
    return err;
}
