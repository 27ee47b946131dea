// ez_capi.hip — implementation of include/eazy.h over the gfx950 kernels: the error strings, the
// token codec and the batch entry points (the streaming handles: ez_writer.hip, ez_reader.hip; the
// multi-device batches: ez_multi.hip; what they share: ez_host.h).  Host-side responsibilities only:
// argument validation (the reference's panics), buffers and copies for the handles' per-call data,
// kernel launches.  All compression and decompression runs in K1/K2/K3; there is no CPU code path.
#include <hip/hip_runtime.h>

#include <stdlib.h>
#include <string.h>

#include <mutex>

#include "ez_cache.h"
#include "ez_format.h"
#include "ez_host.h"
#include "ez_internal.h"

using namespace ez;

int ez::device_count() {
    static std::mutex mu;
    static int count = -1;
    std::lock_guard<std::mutex> lk(mu);
    if (count < 0) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
        count = n;
    }
    return count;
}

namespace {
// K1 scratch (match records / global hash tables / K1c's logs), one per (device, HIP stream), each
// locked only by the call using it: batch calls on distinct streams run concurrently (SURVEY §8b
// threading; ez_cache.h)
ez::DevCache &k1_cache() {
    static ez::DevCache *c = new ez::DevCache();  // (never destroyed: no hipFree after the runtime's teardown)
    return *c;
}
}  // namespace

// ------------------------------------------------------------------ misc

extern "C" const char *ez_strerror(int code) {
    switch (code) {
    case EZ_OK: return "ok";
    case EZ_EOF: return "EOF";
    case EZ_ESHORTBUF: return "short buffer";
    case EZ_EUNEXPECTEDEOF: return "unexpected EOF";
    case EZ_EOVERFLOW: return "length/offset overflow";
    case EZ_EBADMAGIC: return "bad magic";
    case EZ_ENOMAGIC: return "no magic";
    case EZ_EBLOCKLIMIT: return "block size is more than the limit";
    case EZ_EUNSUPMETA: return "unsupported meta tag";
    case EZ_EUNSUPVER: return "unsupported file format version";
    case EZ_EBREAK: return "break point";
    case EZ_EMISSEDMETA: return "missed meta";
    case EZ_EINVAL: return "invalid argument (reference panic)";
    case EZ_ESINK: return "underlying writer failed";
    case EZ_ENOSPC: return "output buffer too small";
    case EZ_EDEVICE: return "no usable MI355X device / HIP error";
    case EZ_ESTUCK: return "kernel progress guard tripped";
    default: return "unknown error";
    }
}

// the value each reference panic carries (writer.go:163, 167, 309/596, 562, 601)
extern "C" const char *ez_panic_message(int panic) {
    switch (panic) {
    case EZ_PANIC_BLOCK: return "block size must be a power of two (32 < bs < 1<<31)";
    case EZ_PANIC_HTABLE: return "hash table size must be a power of two (hs >= 4)";
    case EZ_PANIC_LENGTH: return "too big length";
    case EZ_PANIC_OFFSET: return "too big offset";
    case EZ_PANIC_META: return "meta";  // Go panics with the meta value itself (an int)
    default: return "";
    }
}

// Writer.init writer.go:161-169: the block check comes first
extern "C" int ez_writer_size_panic(int64_t block, int64_t htable) {
    if (((block - 1) & block) != 0 || block < 32 || block > ((int64_t)1 << 31)) return EZ_PANIC_BLOCK;
    if (((htable - 1) & htable) != 0 || htable < 4) return EZ_PANIC_HTABLE;
    return EZ_PANIC_NONE;
}

extern "C" int ez_abi_version(void) { return EZ_ABI_VERSION; }

#ifdef EZ_KNOBS
namespace ez {
const char *knob_str(const char *name) { return getenv(name); }
int knob(const char *name, int dflt) {
    const char *v = getenv(name);
    return v ? atoi(v) : dflt;
}
}  // namespace ez
#endif
extern "C" int ez_device_count(void) { return device_count(); }

// ------------------------------------------------------------------ token codec

// an encoded token of k bytes (k < 0: the encoder refused it) appended to b[*len .. cap)
static int append_token(uint8_t *b, size_t cap, size_t *len, const uint8_t *t, int k) {
    if (k < 0) return EZ_EINVAL;
    if (*len + (size_t)k > cap) return EZ_ENOSPC;
    memcpy(b + *len, t, (size_t)k);
    *len += (size_t)k;
    return EZ_OK;
}

extern "C" int ez_encode_tag(uint8_t *b, size_t cap, size_t *len, int tag, int64_t l) {
    uint8_t t[16];
    return append_token(b, cap, len, t, ez::enc_tag(t, tag, l));
}

extern "C" int ez_encode_offset(uint8_t *b, size_t cap, size_t *len, int64_t off, int64_t l) {
    uint8_t t[16];
    return append_token(b, cap, len, t, ez::enc_offset(t, off, l));
}

extern "C" int ez_encode_meta(uint8_t *b, size_t cap, size_t *len, int64_t meta, int64_t l) {
    uint8_t t[16];
    return append_token(b, cap, len, t, ez::enc_meta(t, meta, l));
}

extern "C" int ez_decode_tag(const uint8_t *b, size_t n, size_t st, int *tag, int64_t *l, size_t *i) {
    int64_t j;
    const int e = ez::dec_tag(b, (int64_t)n, (int64_t)st, tag, l, &j);
    *i = (size_t)j;
    return e;
}

extern "C" int ez_decode_offset(const uint8_t *b, size_t n, size_t st, int64_t l, int64_t *off, size_t *i) {
    int64_t j;
    const int e = ez::dec_offset(b, (int64_t)n, (int64_t)st, l, off, &j);
    *i = (size_t)j;
    return e;
}

extern "C" int ez_decode_meta(const uint8_t *b, size_t n, size_t st, int64_t *meta, int64_t *l, size_t *i) {
    int64_t j;
    const int e = ez::dec_meta(b, (int64_t)n, (int64_t)st, meta, l, &j);
    *i = (size_t)j;
    return e;
}

extern "C" size_t ez_compress_bound(size_t n) { return (size_t)ez::compress_bound(n); }

// ------------------------------------------------------------------ batches

static int compress_batch_impl(int64_t block, int64_t htable, int flags, const ez_batch *b, const uint64_t *write_idx,
                               const uint64_t *write_end, uint64_t max_writes, void *hip_stream) {
    if (!valid_writer_sizes(block, htable)) return EZ_EINVAL;
    if (device_count() <= 0) return EZ_EDEVICE;
    ez::CompressArgs a{};
    a.in = b->in;
    a.in_off = b->in_off;
    a.out = b->out;
    a.out_off = b->out_off;
    a.out_size = b->out_size;
    a.status = b->status;
    a.count = b->count;
    a.bs = block;
    a.hs = htable;
    a.append_magic = (flags & EZ_F_NO_MAGIC) ? 0 : 1;
    a.ver = 0;
    a.header = 1;
    a.start = 0;
    a.ring = nullptr;
    a.max_len = b->max_len;
    a.write_idx = write_idx;
    a.write_end = write_end;
    a.max_writes = max_writes;
    // multi-Write streams: K1s when it takes them (fresh streams, 2 x stream <= block), else the
    // general kernel (one wave per stream, the history read from the stream's earlier Writes)
    if (write_idx && b->count == 0) return EZ_OK;
    // (a forced 'w' keeps them off K1s, as it does single Writes)
    const bool split_mw = write_idx && !ez::compress_forced_general() && ez::split_applies(a);
    auto words_of = [&](const ez::CompressArgs &x) { return split_mw ? ez::split_scratch_words(x) : ez::compress_scratch_words(x); };
    uint64_t words = words_of(a);
    // the scratch of this (device, stream) stays leased through the launches: another host thread
    // growing it meanwhile would free what these kernels were given
    ez::CacheLease lease;
    if (words) {
        int dev = 0;
        EZ_HIP(hipGetDevice(&dev));
        lease = k1_cache().acquire(dev, hip_stream);
        if (!lease->ensure((size_t)words * 4)) {
            // K1c's logs (about 13 bytes per input byte) may not fit where K1L's records do: K1L alone
            ez::CompressArgs b = a;
            b.no_k1c = 1;
            const uint64_t w2 = words_of(b);
            if (w2 >= words || !lease->ensure((size_t)w2 * 4)) return EZ_EDEVICE;
            a = b;
        }
        a.ht_global = (uint32_t *)lease->p;
    }
    if (split_mw) EZ_HIP(ez::launch_compress_split(a, a.ht_global, (hipStream_t)hip_stream));
    else EZ_HIP(ez::launch_compress(a, (hipStream_t)hip_stream));
    return EZ_OK;
}

extern "C" int ez_compress_batch(int64_t block, int64_t htable, int flags, const ez_batch *b, void *hip_stream) {
    return compress_batch_impl(block, htable, flags, b, nullptr, nullptr, 0, hip_stream);
}

extern "C" int ez_compress_batch_writes(int64_t block, int64_t htable, int flags, const ez_batch *b, const uint64_t *write_idx,
                                        const uint64_t *write_end, uint64_t max_writes, void *hip_stream) {
    if (!write_idx || !write_end || max_writes == 0) return EZ_EINVAL;
    return compress_batch_impl(block, htable, flags, b, write_idx, write_end, max_writes, hip_stream);
}

extern "C" size_t ez_pack_workspace(uint64_t count) { return ez::pack_workspace(count); }

extern "C" int ez_pack_batch(const uint8_t *slots, const uint64_t *slot_off, const uint64_t *sizes, uint64_t count,
                             uint8_t *packed, uint64_t *packed_off, void *workspace, void *hip_stream) {
    if (device_count() <= 0) return EZ_EDEVICE;
    EZ_HIP(ez::launch_pack(slots, slot_off, sizes, count, packed, packed_off, workspace, (hipStream_t)hip_stream));
    return EZ_OK;
}

extern "C" int ez_compress_kernel(int64_t block, int64_t htable, uint64_t max_len, uint64_t count) {
    if (!valid_writer_sizes(block, htable)) return -EZ_EINVAL;
    if (device_count() <= 0) return -EZ_EDEVICE;
    ez::CompressArgs a{};
    a.count = count;
    a.bs = block;
    a.hs = htable;
    a.max_len = max_len;
    a.append_magic = 1;
    a.header = 1;
    return (int)ez::compress_variant(a);
}

extern "C" int ez_select_compress_kernel(int kind) {
    if (kind != 0 && !strchr("sSwxl", kind)) return EZ_EINVAL;
    ez::select_split_table(kind == 'S');
    ez::select_compress_variant(kind == 'S' ? 's' : kind);
    return EZ_OK;
}

extern "C" int ez_select_decompress_kernel(int kind) {
    if (kind != 0 && kind != 'r' && kind != 'w' && kind != 't' && kind != 'j') return EZ_EINVAL;
    ez::select_decompress_variant(kind);
    return EZ_OK;
}

extern "C" int ez_decompress_kernel_last(void) { return ez::last_decompress_variant(); }

extern "C" int ez_compress_route_last(char *buf, int cap) {
    const char *r = ez::last_compress_route();
    const int n = (int)strlen(r);
    if (buf && cap > 0) {
        const int k = n < cap - 1 ? n : cap - 1;
        memcpy(buf, r, (size_t)k);
        buf[k] = 0;
    }
    return n;
}

extern "C" int ez_compress_k1c_stats(int enable, uint64_t *counts) {
    ez::k1c_stats(enable, counts);
    return EZ_OK;
}

extern "C" size_t ez_decompress_workspace(uint64_t count) {
    return (size_t)ez::decompress_workspace_words(count) * sizeof(uint32_t);
}

extern "C" int ez_decompress_batch(int64_t block_size_limit, const ez_batch *b, void *workspace, void *hip_stream) {
    if (device_count() <= 0) return EZ_EDEVICE;
    ez::DecompressArgs a{};
    a.in = b->in;
    a.in_off = b->in_off;
    a.out = b->out;
    a.out_off = b->out_off;
    a.out_size = b->out_size;
    a.status = b->status;
    a.count = b->count;
    a.block_size_limit = block_size_limit;
    a.handle = 0;
    a.slow = (uint32_t *)workspace;
    a.max_out = b->max_len;  // decompress: the largest output slot, if the caller knows it
    a.in_bytes = b->in_bytes;  // the batch's extents, if the caller knows them
    a.out_bytes = b->out_bytes;
    EZ_HIP(ez::launch_decompress(a, (hipStream_t)hip_stream));
    return EZ_OK;
}

extern "C" int ez_decompressed_size_batch(int64_t block_size_limit, const ez_batch *b, void *workspace, void *hip_stream) {
    if (device_count() <= 0) return EZ_EDEVICE;
    if (!b->out_size) return EZ_EINVAL;
    ez::DecompressArgs a{};
    a.in = b->in;
    a.in_off = b->in_off;
    a.out_size = b->out_size;
    a.status = b->status;
    a.count = b->count;
    a.block_size_limit = block_size_limit;
    a.slow = (uint32_t *)workspace;
    a.in_bytes = b->in_bytes;  // the batch's input extent, if the caller knows it: the parts route needs it
    EZ_HIP(ez::launch_decompress_size(a, b->max_len, (hipStream_t)hip_stream));
    return EZ_OK;
}

extern "C" int ez_decompressed_size_chunk(uint64_t max_len) { return ez::size_chunk(max_len); }

extern "C" int ez_decompressed_size_chunk_last(void) { return ez::last_size_chunk(); }

extern "C" int ez_select_size_route(int kind) {
    if (kind != 0 && kind != 'p' && kind != 'v') return EZ_EINVAL;
    ez::select_size_route(kind);
    return EZ_OK;
}

extern "C" int ez_decompressed_size_parts_last(uint64_t counts[3]) {
    if (!counts) return EZ_EINVAL;
    counts[0] = counts[1] = counts[2] = 0;
    if (device_count() <= 0) return EZ_EDEVICE;
    EZ_HIP(ez::size_parts_last(counts));
    return EZ_OK;
}

extern "C" int ez_decompressed_size_segs_last(const void *workspace, uint64_t count, uint64_t counts[3]) {
    if (!workspace || !counts) return EZ_EINVAL;
    counts[0] = counts[1] = counts[2] = 0;
    if (device_count() <= 0) return EZ_EDEVICE;
    if (count == 0) return EZ_OK;  // (such a query touches no workspace)
    uint32_t c[3];
    EZ_HIP(hipMemcpy(c, ez::size_segs_counters((uint32_t *)workspace, count), sizeof c, hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; k++) counts[k] = c[k];
    return EZ_OK;
}

// ---- K2g: concatenated streams (ez_decompress_segs.hip)

extern "C" size_t ez_segments_workspace(uint64_t count) { return (size_t)ez::segments_workspace_bytes(count); }

extern "C" int ez_stream_segments_batch(int64_t block_size_limit, const ez_batch *b, uint64_t *seg_idx, uint64_t *seg_in, uint64_t *seg_out,
                                        uint64_t seg_cap, uint64_t *seg_total, void *workspace, void *hip_stream) {
    if (!b || !b->in_off || !b->out_off || !seg_idx || !seg_in || !seg_out || !seg_total || !workspace) return EZ_EINVAL;
    if ((b->count != 0 && !b->in) || seg_cap < b->count) return EZ_EINVAL;
    if (device_count() <= 0) return EZ_EDEVICE;
    ez::SegsArgs a{};
    a.in = b->in;
    a.in_off = b->in_off;
    a.out_off = b->out_off;
    a.count = b->count;
    a.block_size_limit = block_size_limit;
    a.seg_idx = seg_idx;
    a.seg_in = seg_in;
    a.seg_out = seg_out;
    a.seg_cap = seg_cap;
    a.seg_total = seg_total;
    a.in_bytes = b->in_bytes;  // the batch's input extent, if the caller knows it: the parts route needs it
    EZ_HIP(ez::launch_segments(a, b->max_len, workspace, (hipStream_t)hip_stream));
    return EZ_OK;
}

extern "C" int ez_select_segments_route(int kind) {
    if (kind != 0 && kind != 'p' && kind != 'v') return EZ_EINVAL;
    ez::select_segments_route(kind);
    return EZ_OK;
}

extern "C" int ez_segments_parts_last(uint64_t counts[4]) {
    if (!counts) return EZ_EINVAL;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (device_count() <= 0) return EZ_EDEVICE;
    EZ_HIP(ez::segs_parts_last(counts));
    return EZ_OK;
}

extern "C" int ez_segments_merge_batch(const ez_batch *b, const uint64_t *seg_idx, const uint64_t *seg_out, const uint64_t *seg_size,
                                       const int32_t *seg_status, void *hip_stream) {
    if (!b || !b->out_off || !b->out_size || !seg_idx || !seg_out || !seg_size || !seg_status) return EZ_EINVAL;
    if (device_count() <= 0) return EZ_EDEVICE;
    EZ_HIP(ez::launch_segments_merge(b->out_off, b->out_size, b->status, b->count, seg_idx, seg_out, seg_size, seg_status, nullptr, nullptr,
                                     (hipStream_t)hip_stream));
    return EZ_OK;
}

extern "C" int ez_decompress_batch_segmented(int64_t block_size_limit, const ez_batch *b, void *workspace, void *hip_stream) {
    (void)workspace;  // (accepted for symmetry with ez_decompress_batch: the call keeps its own)
    if (!b || !b->in_off || !b->out_off || !b->out_size) return EZ_EINVAL;
    if (device_count() <= 0) return EZ_EDEVICE;
    ez::DecompressArgs a{};
    a.in = b->in;
    a.in_off = b->in_off;
    a.out = b->out;
    a.out_off = b->out_off;
    a.out_size = b->out_size;
    a.status = b->status;
    a.count = b->count;
    a.block_size_limit = block_size_limit;
    a.in_bytes = b->in_bytes;  // the batch's input extent or more, if the caller knows it: the query's parts route needs it
    EZ_HIP(ez::launch_decompress_segmented(a, (hipStream_t)hip_stream));
    return EZ_OK;
}

extern "C" int ez_segments_last(uint64_t counts[3]) {
    if (!counts) return EZ_EINVAL;
    counts[0] = counts[1] = counts[2] = 0;
    if (device_count() <= 0) return EZ_EDEVICE;
    EZ_HIP(ez::segments_last(counts));
    return EZ_OK;
}

// ---- K2b: the Break index (ez_decompress_brk.hip)

extern "C" size_t ez_breaks_workspace(uint64_t count) { return (size_t)ez::breaks_workspace_bytes(count); }

extern "C" int ez_stream_breaks_batch(int64_t block_size_limit, const ez_batch *b, uint64_t *brk_idx, uint64_t *brk_pos, uint64_t brk_cap,
                                      uint64_t *brk_total, void *workspace, void *hip_stream) {
    if (!b || !b->out_size || !brk_idx || !brk_total || (!brk_pos && brk_cap != 0)) return EZ_EINVAL;
    if (b->count != 0 && (!b->in || !b->in_off)) return EZ_EINVAL;
    if (device_count() <= 0) return EZ_EDEVICE;
    ez::BrkArgs a{};
    a.in = b->in;
    a.in_off = b->in_off;
    a.out_size = b->out_size;
    a.status = b->status;
    a.count = b->count;
    a.block_size_limit = block_size_limit;
    a.brk_idx = brk_idx;
    a.brk_pos = brk_pos;
    a.brk_cap = brk_cap;
    a.brk_total = brk_total;
    a.in_bytes = b->in_bytes;  // the batch's input extent or more, if the caller knows it: the parts route needs it
    EZ_HIP(ez::launch_breaks(a, b->max_len, workspace, (hipStream_t)hip_stream));
    return EZ_OK;
}

extern "C" int ez_select_breaks_route(int kind) {
    if (kind != 0 && kind != 'p' && kind != 'v') return EZ_EINVAL;
    ez::select_breaks_route(kind);
    return EZ_OK;
}

extern "C" int ez_breaks_parts_last(uint64_t counts[4]) {
    if (!counts) return EZ_EINVAL;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (device_count() <= 0) return EZ_EDEVICE;
    EZ_HIP(ez::breaks_parts_last(counts));
    return EZ_OK;
}

// Frees the device scratch the batch calls keep between calls (no reference counterpart; like a
// caching allocator's empty_cache): the K1 / K1c scratch and K2j workspaces per (device, HIP stream),
// the multi-device calls' pooled shard buffers, the Reader handles' shared K2j workspace,
// ez_writer_write_many's staging, ez_decompress_batch_segmented's scratch, the segment query's and the Break index's parts-route scratch, on `device` (< 0: every device).  Scratch a call is using at that moment is kept.
extern "C" int ez_release_cached(int device) {
    const int have = device_count();
    if (have <= 0) return EZ_EDEVICE;
    if (device >= have) return EZ_EINVAL;
    DeviceGuard keep(-1);
    for (int d = device < 0 ? 0 : device; d < (device < 0 ? have : device + 1); d++) {
        if (hipSetDevice(d) != hipSuccess) return EZ_EDEVICE;
        k1_cache().trim(d);
        ez::jump_cache().trim(d);
        ez::size_cache().trim(d);
        ez::segs_cache().trim(d);
        ez::segs_parts_cache().trim(d);
        ez::breaks_parts_cache().trim(d);
        reader_release_cached(d);
        writer_release_cached(d);
    }
    multi_release_cached(device);
    return EZ_OK;
}

// Testing: sets the scratch ez_release_cached would free to `byte` (0..255; -1: touches nothing) and
// reports its size in *bytes (may be NULL): the K1 / K1c scratch, K2j workspaces, the three parts routes' and
// ez_decompress_batch_segmented's scratch per (device, HIP stream), ez_writer_write_many's staging
// (device and pinned), the Reader handles' shared K2j workspace and the multi-device calls' pooled
// shard buffers, on `device` (< 0: every device).  Scratch a call is using at that moment is skipped.
// It waits for the device before it fills and before it returns.
extern "C" int ez_fill_cached(int device, int byte, uint64_t *bytes) {
    if (bytes) *bytes = 0;
    const int have = device_count();
    if (have <= 0) return EZ_EDEVICE;
    if (device >= have || byte < -1 || byte > 255) return EZ_EINVAL;
    DeviceGuard keep(-1);
    uint64_t n = 0;
    bool ok = true;
    for (int d = device < 0 ? 0 : device; d < (device < 0 ? have : device + 1); d++) {
        if (hipSetDevice(d) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return EZ_EDEVICE;
        ok &= k1_cache().fill(d, byte, &n);
        ok &= ez::jump_cache().fill(d, byte, &n);
        ok &= ez::size_cache().fill(d, byte, &n);
        ok &= ez::segs_cache().fill(d, byte, &n);
        ok &= ez::segs_parts_cache().fill(d, byte, &n);
        ok &= ez::breaks_parts_cache().fill(d, byte, &n);
        ok &= reader_fill_cached(d, byte, &n);
        ok &= writer_fill_cached(d, byte, &n);
        ok &= multi_fill_cached(d, byte, &n);
        if (hipDeviceSynchronize() != hipSuccess) return EZ_EDEVICE;
    }
    if (bytes) *bytes = n;
    return ok ? EZ_OK : EZ_EDEVICE;
}
