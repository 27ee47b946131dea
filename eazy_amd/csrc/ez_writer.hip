// ez_writer.hip — the Writer handle of include/eazy.h: its ring, table and position in HBM, the
// Writes' staging through pinned host memory, and the K1L / general kernel launches on its stream.
#include <hip/hip_runtime.h>

#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <vector>

#include "ez_cache.h"
#include "ez_format.h"
#include "ez_host.h"
#include "ez_internal.h"

using namespace ez;

struct ez_writer {
    int device = 0;
    int64_t bs = 0, hs = 0;
    int append_magic = 1;
    int ver = 0;
    bool pristine = true;  // isreset(): nothing emitted since the last reset
    // the device's ring and table may hold a Write that failed and was not reset (writer_zero itself
    // failed): the next call resets them first, and fails until that works
    bool tainted = false;
    int64_t pos = 0;       // w.pos
    int last_panic = EZ_PANIC_NONE;  // the reference panic behind the last EZ_EINVAL
    // dev: [input | in_off[2] out_off[2] out_size status write_idx[2] | write_end[k] | write_out[k] | output]
    DBuf ring, ht, dev;
    DBuf recs;             // K1L's match records (single Writes, ez::long_ring_applies)
    HBuf host;             // the same layout, pinned
    uint8_t *host_dev = nullptr;  // the device's address of `host` (zero-copy Writes), or nullptr
    void *host_alias_of = nullptr;  // the host.p host_dev was taken for
    uint32_t seq = 0;               // the zero-copy path's completion flag value of the last Write
    hipStream_t stream = nullptr;
};

namespace {

int writer_zero(ez_writer *w) {
    EZ_HIP(hipMemsetAsync(w->ring.p, 0, (size_t)w->bs, w->stream));
    EZ_HIP(hipMemsetAsync(w->ht.p, 0, (size_t)w->hs * 4, w->stream));
    EZ_HIP(hipStreamSynchronize(w->stream));
    w->pos = 0;
    w->pristine = true;
    w->tainted = false;
    return EZ_OK;
}

// a call that changes the device history starts from a clean one
int writer_clean(ez_writer *w) { return w->tainted ? writer_zero(w) : EZ_OK; }

// ... and so does one that only emits bytes (Header, Break): a tainted handle is reset first
int writer_untaint(ez_writer *w) {
    if (!w->tainted) return EZ_OK;
    DeviceGuard g(w->device);
    if (!g.ok) return EZ_EDEVICE;
    return writer_clean(w);
}

int writer_alloc(ez_writer *w, int64_t bs, int64_t hs) {
    if (w->ring.ensure((size_t)bs)) return EZ_EDEVICE;
    if (w->ht.ensure((size_t)hs * 4)) return EZ_EDEVICE;
    w->bs = bs;
    w->hs = hs;
    return EZ_OK;
}

}  // namespace

extern "C" int ez_writer_new(int64_t block, int64_t htable, int device, ez_writer **out) {
    *out = nullptr;
    if (!valid_writer_sizes(block, htable)) return EZ_EINVAL;
    DeviceGuard g(device);
    if (!g.ok) return EZ_EDEVICE;
    ez_writer *w = new ez_writer();
    w->device = device;
    w->host.flags = hipHostMallocCoherent;
    if (hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking) != hipSuccess) {
        delete w;
        return EZ_EDEVICE;
    }
    int e = writer_alloc(w, block, htable);
    if (!e) e = writer_zero(w);
    if (e) {
        ez_writer_free(w);
        return e;
    }
    *out = w;
    return EZ_OK;
}

extern "C" void ez_writer_free(ez_writer *w) {
    if (!w) return;
    DeviceGuard g(w->device);
    w->ring.release();
    w->ht.release();
    w->dev.release();
    w->recs.release();
    w->host.release();
    if (w->stream) (void)hipStreamDestroy(w->stream);
    delete w;
}

extern "C" int ez_writer_set_append_magic(ez_writer *w, int on) {
    w->append_magic = on ? 1 : 0;
    return EZ_OK;
}

extern "C" int ez_writer_set_version(ez_writer *w, int ver) {
    w->ver = ver;
    return EZ_OK;
}

extern "C" int ez_writer_is_reset(const ez_writer *w) { return w->pristine || w->tainted ? 1 : 0; }

extern "C" int ez_writer_last_panic(const ez_writer *w) { return w->last_panic; }

// testing hook: w.pos of a handle, ring and table unchanged (positions past 2^32)
extern "C" int ez_writer_set_position(ez_writer *w, int64_t pos) {
    if (pos < 0) return EZ_EINVAL;
    w->pos = pos;
    return EZ_OK;
}

namespace {

// Write j of the Writes p holds back to back, Write j ending at p[ends[j]]: its start and length
uint64_t write_start(const uint64_t *ends, size_t j) { return j ? ends[j - 1] : 0; }
uint64_t write_len(const uint64_t *ends, size_t j) { return ends[j] - write_start(ends, j); }

// The handle's args for one launch on its ring and table: one stream in D, its meta block
// [in_off 2][out_off 2][out_size][status] at dm, continuing the handle's stream at position `start`
ez::CompressArgs handle_args(const ez_writer *w, uint8_t *D, uint64_t *dm, bool header, int64_t start, uint64_t max_len) {
    ez::CompressArgs a{};
    a.in = D;
    a.in_off = dm;
    a.out = D;
    a.out_off = dm + 2;
    a.out_size = dm + 4;
    a.status = (int32_t *)(dm + 5);
    a.count = 1;
    a.bs = w->bs;
    a.hs = w->hs;
    a.append_magic = w->append_magic;
    a.ver = w->ver;
    a.header = header ? 1 : 0;
    a.start = start;
    a.ring = w->ring.as<uint8_t>();
    a.ht_global = w->ht.as<uint32_t>();
    a.max_len = max_len;
    return a;
}

// Write j of k through K1L: its own launch, the header on a pristine stream's first
ez::CompressArgs long_args(const ez_writer *w, uint8_t *D, uint64_t *dm, const uint64_t *ends, size_t j) {
    return handle_args(w, D, dm, w->pristine && j == 0, w->pos + (int64_t)write_start(ends, j), write_len(ends, j));
}

// One Write's meta block, six words a launch reads and writes: the Write at [in0, in1) of the staging
// buffer, its output slot of b bytes at o, and the size and status the kernels store
constexpr size_t kMetaWords = 6;
void meta_fill(uint64_t *mj, uint64_t in0, uint64_t in1, uint64_t o, uint64_t b) {
    mj[0] = in0;
    mj[1] = in1;
    mj[2] = o;
    mj[3] = o + b;
    mj[4] = 0;
    mj[5] = 0;
}
size_t meta_size(const uint64_t *mj) { return (size_t)mj[4]; }
int meta_status(const uint64_t *mj) { return (int)(int32_t)(mj[5] & 0xffffffffu); }

// n bytes of Writes have succeeded: the handle's stream goes on after them
void writer_advance(ez_writer *w, size_t n) {
    w->pos += (int64_t)n;
    w->pristine = false;
    w->tainted = false;
}

// Writes that failed after their launch (st: the kernel's status, or EZ_EDEVICE).  The device history
// may already hold p while the stream position does not: start the stream over, as Go does after a
// failed sink write (writer.go:391-393), so later Writes stay exact.  Returns the call's error.
int writer_fail(ez_writer *w, int st, const uint64_t *ends, size_t k) {
    if (st == EZ_EINVAL) {
        // Encoder.Tag panics only for lengths of 2^32 - 8 past its Len4 base (writer.go:558-562),
        // which needs a Write at least that long (never one K1L takes: those are under 2^26 bytes);
        // the only other panic is the distance check (writer.go:308-310)
        const uint64_t tag_limit = ((uint64_t)1 << 32) - 8 + 65916;
        w->last_panic = EZ_PANIC_OFFSET;
        for (size_t j = 0; j < k; j++)
            if (write_len(ends, j) >= tag_limit) w->last_panic = EZ_PANIC_LENGTH;
    }
    const int z = writer_zero(w);
    return z ? z : st;
}

// k Writes (k >= 1) through K1L on the handle's ring and table, one after another on the handle's
// HIP stream (the parse, the token writer and the ring update of each, no host round trip between
// them): one host->device copy, one device->host copy and one synchronisation for all of them.
// Returns -1 when a Write does not qualify (ez::long_ring_applies): the caller takes the general kernel.
int writer_run_long(ez_writer *w, const uint8_t *p, const uint64_t *ends, size_t k, uint8_t *out, size_t cap, uint64_t *out_ends,
                    size_t bound) {
    if (ez::compress_forced_general()) return -1;
    DeviceGuard g(w->device);
    if (!g.ok) return EZ_EDEVICE;
    const size_t n = (size_t)ends[k - 1];
    uint64_t recmax = 0;
    for (size_t j = 0; j < k; j++) {
        const ez::CompressArgs a = long_args(w, nullptr, nullptr, ends, j);
        if (!ez::long_ring_applies(a)) return -1;
        const uint64_t r = ez::long_ring_scratch_bytes(a);
        recmax = r > recmax ? r : recmax;
    }
    // [input | per Write: in_off[2] out_off[2] out_size status | outputs, Write j's at its bound prefix]
    const size_t o_meta = (n + 15) & ~(size_t)15;
    const size_t o_o = (o_meta + kMetaWords * 8 * k + 15) & ~(size_t)15;
    const size_t o_flag = (o_o + bound + 16 + 63) & ~(size_t)63;  // the completion flag (zero-copy path)
    const size_t total = o_flag + 64;
    // Writes K1L stages in LDS (read once): the kernels read them, and write the output, in the pinned
    // host buffer itself -- no host->device and device->host copies (a 100-byte Write's fixed cost)
    bool zc = true;
    for (size_t j = 0; j < k; j++) zc = zc && write_len(ends, j) <= ez::kHandleLdsWrite;
    if (w->host.ensure(total) || w->recs.ensure((size_t)recmax)) return EZ_EDEVICE;
    if (zc && w->host_alias_of != w->host.p) {  // the device's address of the pinned buffer
        void *dp = nullptr;
        if (hipHostGetDevicePointer(&dp, w->host.p, 0) != hipSuccess) {
            (void)hipGetLastError();
            dp = nullptr;
        }
        w->host_dev = (uint8_t *)dp;
        w->host_alias_of = w->host.p;
    }
    zc = zc && w->host_dev != nullptr;
    if (!zc && w->dev.ensure(total)) return EZ_EDEVICE;
    uint8_t *H = w->host.as<uint8_t>(), *D = zc ? w->host_dev : w->dev.as<uint8_t>();
    memcpy(H, p, n);
    uint64_t *m = (uint64_t *)(H + o_meta);
    size_t boff = 0;
    for (size_t j = 0; j < k; j++) {
        const size_t b = ez_compress_bound((size_t)write_len(ends, j));
        meta_fill(m + kMetaWords * j, write_start(ends, j), ends[j], o_o + boff, b);
        boff += b;
    }
    if (!zc) EZ_HIP(hipMemcpyAsync(D, H, o_meta + kMetaWords * 8 * k, hipMemcpyHostToDevice, w->stream));
    w->tainted = true;  // (cleared when the call completes, or by the reset of a failed one)
    hipError_t he = hipSuccess;
    volatile uint32_t *flag = (volatile uint32_t *)(H + o_flag);
    const uint32_t seq = ++w->seq;
    *flag = seq + 1;  // (not the value this call waits for, whatever the buffer held)
    for (size_t j = 0; j < k && he == hipSuccess; j++) {
        ez::CompressArgs a = long_args(w, D, (uint64_t *)(D + o_meta) + kMetaWords * j, ends, j);
        if (zc && j + 1 == k) {  // the last Write's kernel signals its end in the pinned buffer
            a.done_flag = (uint32_t *)(D + o_flag);
            a.done_seq = seq;
        }
        he = ez::launch_long_ring(a, w->recs.as<uint8_t>(), w->stream);
    }
    // (a single Write's route is its launch's; a call of several says how they reached the device)
    if (k > 1) ez::set_compress_route(zc ? "hl:batch zero-copy" : "hl:batch staged");
    if (he == hipSuccess && !zc) he = hipMemcpyAsync(H + o_meta, D + o_meta, o_o - o_meta + bound, hipMemcpyDeviceToHost, w->stream);
    bool seen = false;
    if (he == hipSuccess && zc) {
        // wait by polling the flag (a few microseconds sooner than the runtime's synchronisation); a
        // kernel that does not signal within 100 ms is waited for, and its error reported, by the runtime
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t spin = 0; !(seen = *flag == seq); spin++)
            if ((spin & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(100)) break;
    }
    if (he == hipSuccess && !seen) he = hipStreamSynchronize(w->stream);
    if (he != hipSuccess) return writer_fail(w, EZ_EDEVICE, ends, k);
    int st = EZ_OK;
    size_t got = 0;
    for (size_t j = 0; j < k && !st; j++) {
        st = meta_status(m + kMetaWords * j);
        got += meta_size(m + kMetaWords * j);
    }
    if (!st && got > cap) st = EZ_ENOSPC;  // cannot happen (cap >= the sum of the bounds)
    if (st) return writer_fail(w, st, ends, k);
    size_t at = 0;
    for (size_t j = 0; j < k; j++) {
        const size_t sz = meta_size(m + kMetaWords * j);
        if (sz) memcpy(out + at, H + (size_t)m[kMetaWords * j + 2], sz);
        at += sz;
        if (out_ends) out_ends[j] = at;
    }
    writer_advance(w, n);
    return EZ_OK;
}

// k Writes on the handle in one launch (k = 1: Writer.Write; k > 1: the same Writes in turn):
// p holds them back to back, Write j ending at p[ends[j]]; out receives what each appends to
// w.b, Write j's bytes ending at out[out_ends[j]].  One host->device copy (the Writes and the
// launch metadata, from pinned staging), the general kernel with the handle's ring and table,
// one device->host copy (status, sizes and bytes), one synchronisation.
int writer_run(ez_writer *w, const uint8_t *p, const uint64_t *ends, size_t k, uint8_t *out, size_t cap, uint64_t *out_ends) {
    w->last_panic = EZ_PANIC_NONE;  // (set again only by a failure of this call)
    const size_t n = k ? (size_t)ends[k - 1] : 0;
    size_t bound = 0;
    for (size_t j = 0; j < k; j++) {
        if (ends[j] < write_start(ends, j)) return EZ_EINVAL;
        bound += ez_compress_bound((size_t)write_len(ends, j));
    }
    // checked before anything reaches the device: the kernel advances the handle's ring and table, so a
    // call that could not return its bytes must not run at all (a retry then sees the same history)
    if (cap < bound) return EZ_ENOSPC;
    {
        DeviceGuard g(w->device);
        if (!g.ok) return EZ_EDEVICE;
        const int z = writer_clean(w);
        if (z) return z;
    }
    if (k >= 1) {  // K1L on the handle's ring and table, when every Write qualifies
        const int e = writer_run_long(w, p, ends, k, out, cap, out_ends, bound);
        if (e >= 0) return e;
    }
    DeviceGuard g(w->device);
    if (!g.ok) return EZ_EDEVICE;
    const size_t o_meta = (n + 15) & ~(size_t)15, nm = 8 + 2 * k;  // meta words
    const size_t o_out = o_meta + nm * 8 + ((k > 1 ? k : 0) * 8);
    const size_t total = ((o_out + 15) & ~(size_t)15) + bound + 16;
    if (w->dev.ensure(total) || w->host.ensure(total)) return EZ_EDEVICE;
    const size_t o_o = (o_out + 15) & ~(size_t)15;
    uint8_t *H = w->host.as<uint8_t>(), *D = w->dev.as<uint8_t>();
    if (n) memcpy(H, p, n);
    uint64_t *m = (uint64_t *)(H + o_meta);
    meta_fill(m, 0, n, o_o, bound);
    m[6] = 0; m[7] = k;
    for (size_t j = 0; j < k; j++) m[8 + j] = ends[j];
    EZ_HIP(hipMemcpyAsync(D, H, o_meta + nm * 8, hipMemcpyHostToDevice, w->stream));
    uint64_t *dm = (uint64_t *)(D + o_meta);
    ez::CompressArgs a = handle_args(w, D, dm, w->pristine, w->pos, n ? n : 1);
    if (k > 1) {  // the Writes' ends, and their output ends recorded by the kernel
        a.write_idx = dm + 6;
        a.write_end = dm + 8;
        a.max_writes = k;
        a.write_out = dm + 8 + k;
    }
    // from the launch on, the device history may already hold p: any failure restarts the stream
    // (writer_fail), so later Writes stay exact
    w->tainted = true;
    hipError_t he = ez::launch_compress(a, w->stream);
    // status, sizes and output back at once (the bound, not the exact size: small Writes)
    if (he == hipSuccess)
        he = hipMemcpyAsync(H + o_meta, D + o_meta, o_o - o_meta + bound, hipMemcpyDeviceToHost, w->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(w->stream);
    if (he != hipSuccess) return writer_fail(w, EZ_EDEVICE, ends, k);
    int st = meta_status(m);
    const size_t got = meta_size(m);
    if (!st && got > bound) st = EZ_ENOSPC;  // cannot happen (tests/test_bound.py)
    if (st) return writer_fail(w, st, ends, k);
    if (got) memcpy(out, H + o_o, got);
    if (out_ends) {
        if (k > 1) for (size_t j = 0; j < k; j++) out_ends[j] = m[8 + k + j];
        else if (k == 1) out_ends[0] = got;
    }
    writer_advance(w, n);
    return EZ_OK;
}

// ez_writer_write_many's staging, device buffer and records per (device, HIP stream), leased for the call
ez::DevCache &many_cache() {
    static ez::DevCache *c = new ez::DevCache();  // (never destroyed: no hipFree after the runtime's teardown)
    return *c;
}
std::atomic<uint64_t> g_many_shared{0}, g_many_own{0};  // ez_writer_write_many_last

// Whether handle w's next Write, of n bytes, can share ez_writer_write_many's launch: K1L takes it
// (ez::long_ring_applies) on its LDS path.  a: the Write's args (no buffers yet)
bool many_shares(const ez_writer *w, uint64_t n, ez::CompressArgs &a) {
    a = long_args(w, nullptr, nullptr, &n, 0);
    return !ez::compress_forced_general() && ez::long_ring_applies(a) && n <= ez::kHandleLdsWrite;
}

}  // namespace

void ez::writer_release_cached(int dev) { many_cache().trim(dev); }
bool ez::writer_fill_cached(int dev, int byte, uint64_t *bytes) { return many_cache().fill(dev, byte, bytes); }

extern "C" int ez_writer_write(ez_writer *w, const uint8_t *p, size_t n, uint8_t *out, size_t cap, size_t *out_n) {
    *out_n = 0;
    const uint64_t end = n;
    uint64_t oe = 0;
    const int e = writer_run(w, p, &end, 1, out, cap, &oe);
    if (!e) *out_n = (size_t)oe;
    return e;
}

extern "C" int ez_writer_write_batch(ez_writer *w, const uint8_t *p, const uint64_t *ends, size_t k, uint8_t *out, size_t cap,
                                     uint64_t *out_ends) {
    if (k == 0) return EZ_OK;
    if (!ends || !out_ends) return EZ_EINVAL;
    return writer_run(w, p, ends, k, out, cap, out_ends);
}

// One Write on each of `count` handles.  The Writes K1L takes on its LDS path (many_shares) share one
// launch, a block per handle (ez::launch_long_rings), through one leased staging buffer:
// [those Writes | per handle: in_off[2] out_off[2] out_size status | descriptors | outputs at their bound
// prefixes], one host->device copy, one device->host copy and one synchronisation on the first handle's
// HIP stream (every handle's own stream is idle: each handle call ends synchronised).  Every other Write
// then runs as ez_writer_write does (writer_run); the bytes reach `out` in handle order.
extern "C" int ez_writer_write_many(ez_writer *const *w, size_t count, const uint8_t *p, const uint64_t *ends, uint8_t *out,
                                    size_t cap, uint64_t *out_ends, int32_t *status) {
    if (count == 0) {
        g_many_shared = g_many_own = 0;
        return EZ_OK;
    }
    // the call's refusals, before anything reaches a device or a handle
    if (!w || !ends || !out_ends) return EZ_EINVAL;
    size_t bound = 0;
    for (size_t j = 0; j < count; j++) {
        if (!w[j] || ends[j] < write_start(ends, j) || w[j]->device != w[0]->device) return EZ_EINVAL;
        bound += ez_compress_bound((size_t)write_len(ends, j));
    }
    {
        std::vector<const ez_writer *> s(w, w + count);
        std::sort(s.begin(), s.end());
        if (std::adjacent_find(s.begin(), s.end()) != s.end()) return EZ_EINVAL;
    }
    if (cap < bound) return EZ_ENOSPC;
    DeviceGuard g(w[0]->device);
    if (!g.ok) return EZ_EDEVICE;
    hipStream_t stream = w[0]->stream;

    std::vector<int> st(count, EZ_OK);
    std::vector<size_t> shared;  // the handles of the shared launch, in order
    std::vector<ez::RingDesc> desc;
    uint64_t longest = 0;
    int64_t max_hs = 0;
    size_t nin = 0, sbound = 0;
    for (size_t j = 0; j < count; j++) {
        w[j]->last_panic = EZ_PANIC_NONE;
        if ((st[j] = writer_clean(w[j])) != EZ_OK) continue;
        const uint64_t n = write_len(ends, j);
        ez::CompressArgs a;
        if (!many_shares(w[j], n, a)) continue;
        shared.push_back(j);
        desc.push_back(ez::RingDesc{a.ring, a.ht_global, a.bs, a.hs, a.start, a.header, a.append_magic});
        longest = n > longest ? n : longest;
        max_hs = a.hs > max_hs ? a.hs : max_hs;
        nin += (size_t)n;
        sbound += ez_compress_bound((size_t)n);
    }

    ez::CacheLease lease;
    const size_t ns = shared.size();
    const size_t o_meta = (nin + 15) & ~(size_t)15;
    const size_t o_desc = o_meta + kMetaWords * 8 * ns;
    const size_t o_o = (o_desc + sizeof(ez::RingDesc) * ns + 15) & ~(size_t)15;
    const size_t total = (o_o + sbound + 16 + 255) & ~(size_t)255;  // (the records after it)
    uint8_t *H = nullptr;
    if (ns) {
        lease = many_cache().acquire(w[0]->device, (void *)stream);
        if (!lease->ensure(total + (size_t)ez::long_rings_scratch_bytes(ns, longest)) || !lease->ensure_host(total))
            return EZ_EDEVICE;  // (no handle has been touched)
        H = (uint8_t *)lease->hp;
        uint8_t *D = (uint8_t *)lease->p;
        uint64_t *m = (uint64_t *)(H + o_meta);
        size_t ioff = 0, boff = 0;
        for (size_t s = 0; s < ns; s++) {
            const size_t j = shared[s], n = (size_t)write_len(ends, j), b = ez_compress_bound(n);
            memcpy(H + ioff, p + write_start(ends, j), n);
            meta_fill(m + kMetaWords * s, ioff, ioff + n, o_o + boff, b);
            ioff += n;
            boff += b;
            // from the launch on, the handle's ring and table may hold the Write (cleared by writer_advance,
            // or by the reset of a failed Write)
            w[j]->tainted = true;
        }
        memcpy(H + o_desc, desc.data(), sizeof(ez::RingDesc) * ns);
        hipError_t he = hipMemcpyAsync(D, H, o_o, hipMemcpyHostToDevice, stream);
        if (he == hipSuccess)
            he = ez::launch_long_rings(D, (uint64_t *)(D + o_meta), (const ez::RingDesc *)(D + o_desc), ns, max_hs, longest, D + total,
                                       stream);
        if (he == hipSuccess) he = hipMemcpyAsync(H + o_meta, D + o_meta, o_o - o_meta + sbound, hipMemcpyDeviceToHost, stream);
        if (he == hipSuccess) he = hipStreamSynchronize(stream);
        if (he != hipSuccess) {  // every handle of the launch fails, and restarts its stream
            for (size_t s = 0; s < ns; s++) {
                const uint64_t n = write_len(ends, shared[s]);
                st[shared[s]] = writer_fail(w[shared[s]], EZ_EDEVICE, &n, 1);
            }
        }
    }

    // in handle order: the shared launch's bytes from the staging buffer, the other Writes now
    size_t at = 0, s = 0, own = 0;
    int first = EZ_OK;
    for (size_t j = 0; j < count; j++) {
        const uint64_t n = write_len(ends, j);
        const bool in_launch = s < ns && shared[s] == j;
        int e = st[j];
        size_t sz = 0;
        if (!e && in_launch) {
            const uint64_t *mj = (const uint64_t *)(H + o_meta) + kMetaWords * s;
            e = meta_status(mj);
            sz = meta_size(mj);
            if (!e && sz > (size_t)(mj[3] - mj[2])) e = EZ_ENOSPC;  // cannot happen (tests/test_bound.py)
            if (e) {
                e = writer_fail(w[j], e, &n, 1);
            } else {
                if (sz) memcpy(out + at, H + (size_t)mj[2], sz);
                writer_advance(w[j], (size_t)n);
            }
        } else if (!e) {
            uint64_t oe = 0;
            e = writer_run(w[j], p + write_start(ends, j), &n, 1, out + at, cap - at, &oe);
            sz = (size_t)oe;
            own++;
        }
        s += in_launch;
        if (!e) at += sz;
        out_ends[j] = at;
        if (status) status[j] = e;
        if (e && !first) first = e;
    }
    g_many_shared = ns;
    g_many_own = own;
    ez::set_compress_route(own == 0 ? "hm:lds" : (ns == 0 ? "hm:own" : "hm:lds+own"));
    return first;
}

extern "C" int ez_writer_write_many_last(uint64_t counts[2]) {
    counts[0] = g_many_shared;
    counts[1] = g_many_own;
    return EZ_OK;
}

extern "C" int ez_writer_header(ez_writer *w, uint8_t *out, size_t cap, size_t *out_n) {
    *out_n = 0;
    const int z = writer_untaint(w);
    if (z) return z;
    if (!w->pristine) return EZ_OK;
    uint8_t h[16];
    const size_t k = header_bytes(h, w->append_magic, w->ver, w->bs);
    if (k > cap) return EZ_ENOSPC;
    memcpy(out, h, k);
    *out_n = k;
    w->pristine = false;
    return EZ_OK;
}

extern "C" int ez_writer_break(ez_writer *w, uint8_t *out, size_t cap, size_t *out_n) {
    *out_n = 0;
    const int z = writer_untaint(w);
    if (z) return z;
    uint8_t h[32];
    size_t k = 0;
    if (w->pristine) k = header_bytes(h, w->append_magic, w->ver, w->bs);
    h[k++] = 0x80;
    h[k++] = 0x18 | 7;  // Meta, MetaBreak|MetaLen0 (writer.go:363)
    if (k > cap) return EZ_ENOSPC;
    memcpy(out, h, k);
    *out_n = k;
    w->pristine = false;
    return EZ_OK;
}

extern "C" int ez_writer_reset(ez_writer *w) {
    DeviceGuard g(w->device);
    if (!g.ok) return EZ_EDEVICE;
    return writer_zero(w);
}

extern "C" int ez_writer_reset_size(ez_writer *w, int64_t block, int64_t htable) {
    if (!valid_writer_sizes(block, htable)) return EZ_EINVAL;
    DeviceGuard g(w->device);
    if (!g.ok) return EZ_EDEVICE;
    int e = writer_alloc(w, block, htable);
    if (e) return e;
    return writer_zero(w);
}
