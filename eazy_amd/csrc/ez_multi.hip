// ez_multi.hip — host batches over several devices (ez_compress_batch_multi,
// ez_decompress_batch_multi, ez_decompressed_size_batch_multi): contiguous shards of whole streams, one host thread and one pooled HIP
// stream per shard, each running the single-device batch calls of ez_capi.hip.
#include <hip/hip_runtime.h>

#include <array>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "ez_format.h"
#include "ez_host.h"
#include "ez_multi_shards.h"

using namespace ez;

namespace {
int resolve_devices(const int *devices, int ndev, std::vector<int> &out) {
    const int have = device_count();
    if (have <= 0) return EZ_EDEVICE;
    if (!devices || ndev <= 0) {
        for (int d = 0; d < have; d++) out.push_back(d);
        return EZ_OK;
    }
    for (int k = 0; k < ndev; k++) {
        if (devices[k] < 0 || devices[k] >= have) return EZ_EINVAL;
        out.push_back(devices[k]);
    }
    return EZ_OK;
}

// A shard's HIP stream, timing events and grow-only device buffers, pooled per device between calls:
// the K1 / K2j scratch caches are keyed by (device, stream), so pooled streams reuse their entries
// instead of leaving one behind per call, and repeated calls do not re-allocate (ez_release_cached
// frees the idle ones).
struct ShardRes {
    int dev = 0;
    hipStream_t st = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // around the shard's device work
    DBuf in, in_off, out, out_off, size, status, ws, packed, packed_off;
    std::array<DBuf *, 9> bufs() { return {&in, &in_off, &out, &out_off, &size, &status, &ws, &packed, &packed_off}; }
    void release_bufs() {
        for (DBuf *b : bufs()) b->release();
    }
};

class ShardPool {
  public:
    // an idle resource of dev, or a new one (the caller's thread is bound to dev); nullptr on failure
    ShardRes *take(int dev) {
        {
            std::lock_guard<std::mutex> lk(m_);
            auto &v = idle_[dev];
            if (!v.empty()) {
                ShardRes *r = v.back();
                v.pop_back();
                return r;
            }
        }
        ShardRes *r = new ShardRes();
        r->dev = dev;
        if (hipStreamCreateWithFlags(&r->st, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&r->ev0) != hipSuccess ||
            hipEventCreate(&r->ev1) != hipSuccess) {
            if (r->ev0) (void)hipEventDestroy(r->ev0);
            if (r->st) (void)hipStreamDestroy(r->st);
            delete r;
            return nullptr;
        }
        return r;
    }
    void give(ShardRes *r) {
        std::lock_guard<std::mutex> lk(m_);
        idle_[r->dev].push_back(r);
    }
    // free the idle resources' buffers on dev (all devices for dev < 0); streams and events stay
    void trim(int dev) {
        std::lock_guard<std::mutex> lk(m_);
        for (auto &kv : idle_) {
            if (dev >= 0 && kv.first != dev) continue;
            if (hipSetDevice(kv.first) != hipSuccess) continue;
            for (ShardRes *r : kv.second) r->release_bufs();
        }
    }
    // set the idle resources' buffers on dev to `byte` (< 0: count only); their bytes are added to *bytes
    bool fill(int dev, int byte, uint64_t *bytes) {
        std::lock_guard<std::mutex> lk(m_);
        bool ok = true;
        for (auto &kv : idle_) {
            if (dev >= 0 && kv.first != dev) continue;
            if (hipSetDevice(kv.first) != hipSuccess) continue;
            for (ShardRes *r : kv.second)
                for (DBuf *b : r->bufs()) {
                    if (!b->p) continue;
                    if (byte >= 0 && hipMemset(b->p, byte, b->cap) != hipSuccess) ok = false;
                    *bytes += b->cap;
                }
        }
        return ok;
    }

  private:
    std::mutex m_;
    std::map<int, std::vector<ShardRes *>> idle_;
};
ShardPool &shard_pool() {
    static ShardPool *p = new ShardPool();  // (never destroyed: no HIP calls after the runtime's teardown)
    return *p;
}

// one shard of a multi-device call (its host thread runs it on a pooled resource)
struct Shard {
    int dev = 0;
    uint64_t first = 0, count = 0;
    ShardRes *r = nullptr;
    uint64_t total = 0, base = 0;  // compress: packed bytes of the shard, its place in the global packing
    int err = EZ_OK;
    ~Shard() {
        if (r) shard_pool().give(r);
    }
};
using Shards = std::vector<std::unique_ptr<Shard>>;

// the batch's shards, one per device of devs in turn
Shards make_shards(const uint64_t *in_off, uint64_t count, const std::vector<int> &devs) {
    const std::vector<uint64_t> first = shard_bounds(in_off, count, (int)devs.size());
    Shards sh;
    for (size_t k = 0; k < devs.size(); k++) {
        sh.emplace_back(new Shard());
        sh[k]->dev = devs[k];
        sh[k]->first = first[k];
        sh[k]->count = first[k + 1] - first[k];
    }
    return sh;
}

// a shard's c + 1 offsets, from its first stream's (ez_multi_shards.h)
std::vector<uint64_t> rebased(const uint64_t *off, const Shard &x) { return ez::rebased(off, x.first, x.count); }

// the per-shard device intervals of the last multi-device call (ez_multi_last_shards)
struct ShardTime {
    int dev;
    double t0, t1;
};
std::mutex g_times_mu;
std::vector<ShardTime> g_times;

// a shard's host thread: it binds its device, takes a pooled resource, and runs f between the events
template <class F>
int run_shard(Shard &x, F &f) {
    EZ_HIP(hipSetDevice(x.dev));
    if (!x.r && !(x.r = shard_pool().take(x.dev))) return EZ_EDEVICE;
    if (x.err != EZ_OK) return x.err;
    EZ_HIP(hipEventRecord(x.r->ev0, x.r->st));
    const int e = f(x);
    if (e != EZ_OK) return e;
    EZ_HIP(hipEventRecord(x.r->ev1, x.r->st));
    EZ_HIP(hipEventSynchronize(x.r->ev1));
    return EZ_OK;
}

// run f(shard) on one host thread per shard, join them, then record their device intervals
template <class F>
int each_shard(Shards &sh, F f, bool record = true) {
    std::vector<std::thread> th;
    for (auto &p : sh) {
        Shard *x = p.get();
        if (x->count) th.emplace_back([x, &f]() { x->err = run_shard(*x, f); });
    }
    for (auto &t : th) t.join();
    for (auto &p : sh)
        if (p->err != EZ_OK) return p->err;
    if (!record) return EZ_OK;
    // device intervals, in ms from the earliest shard start on the same device
    std::vector<ShardTime> tv;
    for (auto &p : sh) {
        if (!p->r || p->count == 0) continue;
        const Shard *ref = nullptr;
        for (auto &q : sh) {  // the shard on this device whose start is earliest
            if (!q->r || q->count == 0 || q->dev != p->dev) continue;
            if (!ref) {
                ref = q.get();
                continue;
            }
            float e = 0.f;
            if (hipSetDevice(p->dev) == hipSuccess && hipEventElapsedTime(&e, ref->r->ev0, q->r->ev0) == hipSuccess && e < 0.f) ref = q.get();
        }
        float a = 0.f, b = 0.f;
        if (hipSetDevice(p->dev) != hipSuccess || hipEventElapsedTime(&a, ref->r->ev0, p->r->ev0) != hipSuccess ||
            hipEventElapsedTime(&b, ref->r->ev0, p->r->ev1) != hipSuccess)
            a = b = -1.f;
        tv.push_back(ShardTime{p->dev, (double)a, (double)b});
    }
    std::lock_guard<std::mutex> lk(g_times_mu);
    g_times.swap(tv);
    return EZ_OK;
}
}  // namespace

void ez::multi_release_cached(int device) { shard_pool().trim(device); }
bool ez::multi_fill_cached(int device, int byte, uint64_t *bytes) { return shard_pool().fill(device, byte, bytes); }

// Introspection (tests, measurement): the shards of the last multi-device call and their device
// intervals (ms from the earliest shard start on the same device; -1 if not measurable)
extern "C" int ez_multi_last_shards(int *dev, double *t0, double *t1, int cap) {
    std::lock_guard<std::mutex> lk(g_times_mu);
    const int n = (int)g_times.size();
    for (int k = 0; k < n && k < cap; k++) {
        if (dev) dev[k] = g_times[(size_t)k].dev;
        if (t0) t0[k] = g_times[(size_t)k].t0;
        if (t1) t1[k] = g_times[(size_t)k].t1;
    }
    return n;
}

extern "C" int ez_compress_batch_multi(int64_t block, int64_t htable, int flags, const uint8_t *in, const uint64_t *in_off,
                                       uint64_t count, const int *devices, int ndev, uint8_t *packed, uint64_t packed_cap,
                                       uint64_t *packed_off, int32_t *status) {
    if (!valid_writer_sizes(block, htable) || !in_off || !packed_off) return EZ_EINVAL;
    if (!offsets_ascend(in_off, count)) return EZ_EINVAL;  // (nothing written, packed_off[0] neither)
    std::vector<int> devs;
    int e = resolve_devices(devices, ndev, devs);
    if (e != EZ_OK) return e;
    packed_off[0] = 0;
    if (count == 0) return EZ_OK;
    DeviceGuard keep(-1);  // (the shards' buffers are freed on this thread, each on its device)
    try {
        Shards sh = make_shards(in_off, count, devs);
        // phase 1: per shard, upload, K1 into bound-sized slots, K3 into a packed shard; its sizes back
        e = each_shard(sh, [&](Shard &x) -> int {
            const uint64_t c = x.count, base = in_off[x.first];
            const std::vector<uint64_t> ioff = rebased(in_off, x);
            const uint64_t nb = ioff[c], mx = max_span(ioff);
            std::vector<uint64_t> ooff(c + 1);
            ooff[0] = 0;
            for (uint64_t t = 0; t < c; t++) ooff[t + 1] = ooff[t] + ((ez_compress_bound(ioff[t + 1] - ioff[t]) + 15) & ~15ull);
            if (x.r->in.ensure(nb + 64) || x.r->in_off.ensure(8 * (c + 1)) || x.r->out.ensure(ooff[c] + 64) || x.r->out_off.ensure(8 * (c + 1)) ||
                x.r->size.ensure(8 * c) || x.r->status.ensure(4 * c) || x.r->ws.ensure(ez_pack_workspace(c) + 64) || x.r->packed.ensure(ooff[c] + 64) ||
                x.r->packed_off.ensure(8 * (c + 1)))
                return EZ_EDEVICE;
            if (nb) EZ_HIP(hipMemcpyAsync(x.r->in.p, in + base, nb, hipMemcpyHostToDevice, x.r->st));
            EZ_HIP(hipMemcpyAsync(x.r->in_off.p, ioff.data(), 8 * (c + 1), hipMemcpyHostToDevice, x.r->st));
            EZ_HIP(hipMemcpyAsync(x.r->out_off.p, ooff.data(), 8 * (c + 1), hipMemcpyHostToDevice, x.r->st));
            ez_batch b{x.r->in.as<uint8_t>(), x.r->in_off.as<uint64_t>(), x.r->out.as<uint8_t>(), x.r->out_off.as<uint64_t>(),
                       x.r->size.as<uint64_t>(), x.r->status.as<int32_t>(), c, mx};
            int r = ez_compress_batch(block, htable, flags, &b, x.r->st);
            if (r != EZ_OK) return r;
            r = ez_pack_batch(x.r->out.as<uint8_t>(), x.r->out_off.as<uint64_t>(), x.r->size.as<uint64_t>(), c, x.r->packed.as<uint8_t>(),
                              x.r->packed_off.as<uint64_t>(), x.r->ws.p, x.r->st);
            if (r != EZ_OK) return r;
            // the shard's packed offsets straight into the caller's array (rebased below; its last one,
            // the shard's total, is the next shard's first entry and comes back separately)
            EZ_HIP(hipMemcpyAsync(packed_off + x.first, x.r->packed_off.p, 8 * c, hipMemcpyDeviceToHost, x.r->st));
            EZ_HIP(hipMemcpyAsync(&x.total, x.r->packed_off.as<uint64_t>() + c, 8, hipMemcpyDeviceToHost, x.r->st));
            if (status) EZ_HIP(hipMemcpyAsync(status + x.first, x.r->status.p, 4 * c, hipMemcpyDeviceToHost, x.r->st));
            EZ_HIP(hipStreamSynchronize(x.r->st));
            return EZ_OK;
        });
        if (e != EZ_OK) return e;
        // the global packing: shard k starts where shard k-1 ends (a host exclusive scan of the totals)
        uint64_t at = 0;
        for (auto &x : sh) {
            x->base = at;
            at += x->total;
            for (uint64_t t = 0; t < x->count; t++) packed_off[x->first + t] += x->base;
        }
        packed_off[count] = at;
        if (at > packed_cap) return EZ_ENOSPC;
        // phase 2: every shard's packed bytes down to its place
        return each_shard(sh, [&](Shard &x) -> int {
            if (x.total) EZ_HIP(hipMemcpyAsync(packed + x.base, x.r->packed.p, x.total, hipMemcpyDeviceToHost, x.r->st));
            EZ_HIP(hipStreamSynchronize(x.r->st));
            return EZ_OK;
        }, false);
    } catch (...) {
        return EZ_EDEVICE;  // (host allocation failure: nothing unwinds across the C-ABI)
    }
}

extern "C" int ez_decompress_batch_multi(int64_t block_size_limit, const uint8_t *in, const uint64_t *in_off, uint64_t count,
                                         const int *devices, int ndev, uint8_t *out, const uint64_t *out_off, uint64_t *out_size,
                                         int32_t *status) {
    if (!in_off || !out_off || !out_size) return EZ_EINVAL;
    if (!offsets_ascend(in_off, count) || !offsets_ascend(out_off, count)) return EZ_EINVAL;
    std::vector<int> devs;
    int e = resolve_devices(devices, ndev, devs);
    if (e != EZ_OK) return e;
    if (count == 0) return EZ_OK;
    DeviceGuard keep(-1);
    try {
        Shards sh = make_shards(in_off, count, devs);
        return each_shard(sh, [&](Shard &x) -> int {
            const uint64_t c = x.count, ib = in_off[x.first], ob = out_off[x.first];
            const std::vector<uint64_t> ioff = rebased(in_off, x), ooff = rebased(out_off, x);
            const uint64_t nb = ioff[c], no = ooff[c], mx = max_span(ooff);
            if (x.r->in.ensure(nb + 64) || x.r->in_off.ensure(8 * (c + 1)) || x.r->out.ensure(no + 64) || x.r->out_off.ensure(8 * (c + 1)) ||
                x.r->size.ensure(8 * c) || x.r->status.ensure(4 * c) || x.r->ws.ensure(ez_decompress_workspace(c) + 64))
                return EZ_EDEVICE;
            if (nb) EZ_HIP(hipMemcpyAsync(x.r->in.p, in + ib, nb, hipMemcpyHostToDevice, x.r->st));
            EZ_HIP(hipMemcpyAsync(x.r->in_off.p, ioff.data(), 8 * (c + 1), hipMemcpyHostToDevice, x.r->st));
            EZ_HIP(hipMemcpyAsync(x.r->out_off.p, ooff.data(), 8 * (c + 1), hipMemcpyHostToDevice, x.r->st));
            // (the largest slot and the extents given: the decoder route needs no device read-back)
            ez_batch b{x.r->in.as<uint8_t>(), x.r->in_off.as<uint64_t>(), x.r->out.as<uint8_t>(), x.r->out_off.as<uint64_t>(),
                       x.r->size.as<uint64_t>(), x.r->status.as<int32_t>(), c, mx ? mx : 1, nb, no};
            const int r = ez_decompress_batch(block_size_limit, &b, x.r->ws.p, x.r->st);
            if (r != EZ_OK) return r;
            if (no) EZ_HIP(hipMemcpyAsync(out + ob, x.r->out.p, no, hipMemcpyDeviceToHost, x.r->st));
            EZ_HIP(hipMemcpyAsync(out_size + x.first, x.r->size.p, 8 * c, hipMemcpyDeviceToHost, x.r->st));
            if (status) EZ_HIP(hipMemcpyAsync(status + x.first, x.r->status.p, 4 * c, hipMemcpyDeviceToHost, x.r->st));
            EZ_HIP(hipStreamSynchronize(x.r->st));
            return EZ_OK;
        });
    } catch (...) {
        return EZ_EDEVICE;
    }
}

// The decoded sizes of a host batch (K2z per shard): the shards, pooled resources and per-shard threads
// of ez_decompress_batch_multi, without an output.
extern "C" int ez_decompressed_size_batch_multi(int64_t block_size_limit, const uint8_t *in, const uint64_t *in_off, uint64_t count,
                                                const int *devices, int ndev, uint64_t *out_size, int32_t *status) {
    if (!in_off || !out_size) return EZ_EINVAL;
    if (!offsets_ascend(in_off, count)) return EZ_EINVAL;
    std::vector<int> devs;
    int e = resolve_devices(devices, ndev, devs);
    if (e != EZ_OK) return e;
    if (count == 0) return EZ_OK;
    DeviceGuard keep(-1);
    try {
        Shards sh = make_shards(in_off, count, devs);
        return each_shard(sh, [&](Shard &x) -> int {
            const uint64_t c = x.count, ib = in_off[x.first];
            const std::vector<uint64_t> ioff = rebased(in_off, x);
            const uint64_t nb = ioff[c], mx = max_span(ioff);
            if (x.r->in.ensure(nb + 64) || x.r->in_off.ensure(8 * (c + 1)) || x.r->size.ensure(8 * c) || x.r->status.ensure(4 * c) ||
                x.r->ws.ensure(ez_decompress_workspace(c) + 64))
                return EZ_EDEVICE;
            if (nb) EZ_HIP(hipMemcpyAsync(x.r->in.p, in + ib, nb, hipMemcpyHostToDevice, x.r->st));
            EZ_HIP(hipMemcpyAsync(x.r->in_off.p, ioff.data(), 8 * (c + 1), hipMemcpyHostToDevice, x.r->st));
            // (the longest input stream and the shard's input bytes given: the query's route needs no read-back)
            ez_batch b{x.r->in.as<uint8_t>(), x.r->in_off.as<uint64_t>(), nullptr, nullptr, x.r->size.as<uint64_t>(), x.r->status.as<int32_t>(),
                       c, mx, nb, 0};
            const int r = ez_decompressed_size_batch(block_size_limit, &b, x.r->ws.p, x.r->st);
            if (r != EZ_OK) return r;
            EZ_HIP(hipMemcpyAsync(out_size + x.first, x.r->size.p, 8 * c, hipMemcpyDeviceToHost, x.r->st));
            if (status) EZ_HIP(hipMemcpyAsync(status + x.first, x.r->status.p, 4 * c, hipMemcpyDeviceToHost, x.r->st));
            EZ_HIP(hipStreamSynchronize(x.r->st));
            return EZ_OK;
        });
    } catch (...) {
        return EZ_EDEVICE;
    }
}
