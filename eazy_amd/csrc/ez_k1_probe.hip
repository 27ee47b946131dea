// ez_k1_probe.hip — the LDS lane-order properties the K1 kernels rely on, each checked once per
// process on the device by a 64-lane probe kernel.
#include "ez_k1_internal.h"

namespace ez {
namespace {
using namespace k1;

// The property T16 relies on, checked once per process on the device:
// same-address ds_write_b16 of one wave instruction land in ascending lane
// order (the highest lane's value stays).
__global__ void k_lds_store_order(uint32_t *res) {
    __shared__ uint16_t t[8];
    const uint32_t l = threadIdx.x;
    if (l < 8) t[l] = 0;
    __syncthreads();
    t[l & 7] = (uint16_t)(l + 1);
    __syncthreads();
    if (l < 8 && t[l] != (uint16_t)(56 + l + 1)) atomicAdd(res, 1u);
}

// the same for 32-bit stores (k1_long's u32 table)
__global__ void k_lds_store_order32(uint32_t *res) {
    __shared__ uint32_t t[8];
    const uint32_t l = threadIdx.x;
    if (l < 8) t[l] = 0;
    __syncthreads();
    t[l & 7] = l + 1;
    __syncthreads();
    if (l < 8 && t[l] != 56 + l + 1) atomicAdd(res, 1u);
}

// The property k1_lean relies on, checked once per process on the device: same-word
// ds_mskor_rtn_b32 of one wave instruction apply in ascending lane order (each lane reads the
// entry as the latest earlier lane on it left it), on both halves of a word.
__global__ void k_lds_mskor_order(uint32_t *res) {
    __shared__ uint16_t t[8];
    const uint32_t l = threadIdx.x;
    if (l < 8) t[l] = 0;
    __syncthreads();
    const uint32_t e = (l * 5 + (l >> 3)) & 7;
    const uint32_t got = lds_mskor16(t, e, l + 1);
    uint32_t want = 0, last = 0;
    for (uint32_t k = 0; k < 64; k++) {
        const uint32_t ek = (k * 5 + (k >> 3)) & 7;
        if (ek == e && k < l) want = k + 1;
        if (l < 8 && ek == l) last = k + 1;
    }
    __syncthreads();
    if (got != want || (l < 8 && t[l] != last)) atomicAdd(res, 1u);
}

// The property T32 relies on, checked once per process on the device: same-address LDS
// exchanges of one wave instruction apply in ascending lane order (lane l reads what lane l-4
// wrote).  If it ever fails, K1s-T32 is not used.
__global__ void k_lds_order(uint32_t *res) {
    __shared__ uint32_t t[4];
    const uint32_t l = threadIdx.x;
    if (l < 4) t[l] = 0;
    __syncthreads();
    const uint32_t old = atomicExch(&t[l & 3], l + 1);
    const uint32_t want = l < 4 ? 0 : l - 3;
    if (old != want) atomicAdd(res, 1u);
}

// one 64-lane probe kernel on a private stream; true when it reports no violation
bool lds_probe(void (*kern)(uint32_t *)) {
    uint32_t *d = nullptr, h = 1;
    hipStream_t st = nullptr;
    bool ok = false;
    if (hipMalloc(&d, sizeof(uint32_t)) != hipSuccess) return false;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess) {
        if (hipMemsetAsync(d, 0, sizeof(uint32_t), st) == hipSuccess) {
            hipLaunchKernelGGL(kern, dim3(1), dim3(64), 0, st, d);
            if (hipGetLastError() == hipSuccess && hipMemcpyAsync(&h, d, sizeof(uint32_t), hipMemcpyDeviceToHost, st) == hipSuccess &&
                hipStreamSynchronize(st) == hipSuccess)
                ok = h == 0;
        }
        (void)hipStreamDestroy(st);
    }
    (void)hipFree(d);
    return ok;
}

}  // namespace

bool lds_exchange_in_lane_order() {
    static const bool ok = lds_probe(k_lds_order);
    return ok;
}

bool lds_store_in_lane_order() {
    static const bool ok = lds_probe(k_lds_store_order);
    return ok;
}

bool lds_mskor_in_lane_order() {
    static const bool ok = lds_probe(k_lds_mskor_order);
    return ok;
}

bool lds_store32_in_lane_order() {
    static const bool ok = lds_probe(k_lds_store_order32);
    return ok;
}

}  // namespace ez
