// ez_host.h — what the host-side sources of the C-ABI share (ez_capi.hip, ez_writer.hip,
// ez_reader.hip, ez_multi.hip): the device guard, the grow-only buffers, the Writer's size checks
// and header bytes, and the few hooks one of those files offers the others.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "ez_format.h"

namespace ez {

int device_count();  // (ez_capi.hip; 0 when the runtime reports none)

// ez_release_cached's part in the file that owns the scratch; the caller's thread is bound to dev
void reader_release_cached(int dev);    // the Readers' shared K2j workspace of dev, unless one is using it
void multi_release_cached(int device);  // the idle shard buffers of device (< 0: every device)
void writer_release_cached(int dev);    // ez_writer_write_many's idle staging, device buffers and records of dev
// ez_fill_cached's part beside each: the same buffers set to `byte` (< 0: counted only), their bytes
// added to *bytes; false when a hipMemset failed
bool reader_fill_cached(int dev, int byte, uint64_t *bytes);
bool multi_fill_cached(int device, int byte, uint64_t *bytes);
bool writer_fill_cached(int dev, int byte, uint64_t *bytes);

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (device_count() <= 0) return;
        if (hipGetDevice(&prev) != hipSuccess) return;
        if (dev >= 0 && dev != prev && hipSetDevice(dev) != hipSuccess) return;
        ok = true;
    }
    ~DeviceGuard() {
        if (ok && prev >= 0) (void)hipSetDevice(prev);
    }
};

#define EZ_HIP(x)                                   \
    do {                                            \
        if ((x) != hipSuccess) return EZ_EDEVICE;   \
    } while (0)

// where a grow-only buffer lives: device memory, or pinned host staging (one copy each way per
// call, no pageable bounce)
struct DeviceMem {
    static constexpr size_t kMin = 4096;
    static hipError_t alloc(void **p, size_t n, unsigned) { return hipMalloc(p, n); }
    static hipError_t dealloc(void *p) { return hipFree(p); }
};
struct PinnedMem {
    static constexpr size_t kMin = 65536;
    static hipError_t alloc(void **p, size_t n, unsigned flags) { return hipHostMalloc(p, n, flags); }
    static hipError_t dealloc(void *p) { return hipHostFree(p); }
};

// grow-only buffer (+ 25 %; the contents are not kept)
template <class Mem>
struct Buf {
    void *p = nullptr;
    size_t cap = 0;
    unsigned flags = hipHostMallocDefault;  // (PinnedMem only; a Writer's: coherent, the kernels read and write it in place)
    int ensure(size_t n) {
        if (n <= cap) return EZ_OK;
        release();
        size_t c = n < Mem::kMin ? Mem::kMin : n + n / 4;
        if (Mem::alloc(&p, c, flags) != hipSuccess) return EZ_EDEVICE;
        cap = c;
        return EZ_OK;
    }
    void release() {
        if (p) (void)Mem::dealloc(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T *as() const { return (T *)p; }
};
using DBuf = Buf<DeviceMem>;
using HBuf = Buf<PinnedMem>;

// Writer.init size checks (writer.go:161-169)
inline bool valid_writer_sizes(int64_t bs, int64_t hs) { return ez_writer_size_panic(bs, hs) == EZ_PANIC_NONE; }

// appendHeader writer.go:495-517
inline size_t header_bytes(uint8_t *b, int append_magic, int ver, int64_t bs) {
    size_t k = 0;
    if (append_magic) {
        const uint8_t m[6] = {0x80, 0x02, 'e', 'a', 'z', 'y'};
        memcpy(b, m, 6);
        k = 6;
    }
    if (ver != 0) {
        b[k++] = 0x80; b[k++] = 0x08; b[k++] = (uint8_t)ver;
    }
    b[k++] = 0x80; b[k++] = 0x10; b[k++] = (uint8_t)__builtin_ctzll((uint64_t)bs);
    return k;
}

}  // namespace ez
