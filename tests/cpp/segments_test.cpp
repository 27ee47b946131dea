// eazy::DecompressBatchSegmented (eazy_amd/cpp/eazy.hpp): 64 streams of 4 compressed streams joined back
// to back, about 8 KiB of output each, round trip: the plain bytes come back, every one of the 256
// segments was decoded by a fast decoder, and the query needed no retry.  Needs a device.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <string>
#include <vector>

#include "../../eazy_amd/cpp/eazy.hpp"

namespace {

std::vector<uint8_t> text(size_t n, int salt) {
    std::vector<uint8_t> v;
    for (size_t k = 0; v.size() < n; k++) {
        const std::string s = "2026-01-01T00:00:00 INFO tenant-" + std::to_string((k * 7 + (size_t)salt) % 13) + " GET /api/v1/items/" +
                              std::to_string(k * 31 + (size_t)salt) + " status=200\n";
        v.insert(v.end(), s.begin(), s.end());
    }
    v.resize(n);
    return v;
}

#define HIP_OK(x)                                   \
    do {                                            \
        if ((x) != hipSuccess) {                    \
            printf("FAIL: %s\n", #x);               \
            return 1;                               \
        }                                           \
    } while (0)

}  // namespace

int main() {
    using namespace eazy;
    const size_t streams = 64, segs = 4;
    std::vector<std::vector<uint8_t>> plain, comp;
    for (size_t k = 0; k < streams * segs; k++) plain.push_back(text(8000 + 37 * (k % 11), (int)k));
    if (CompressBatchMulti(plain, 1 << 20, 1024, comp, {0}) != Err::OK) {
        printf("FAIL: compress\n");
        return 1;
    }
    std::vector<uint8_t> in, want;
    std::vector<uint64_t> in_off{0}, out_off{0};
    for (size_t s = 0; s < streams; s++) {
        for (size_t g = 0; g < segs; g++) {
            in.insert(in.end(), comp[s * segs + g].begin(), comp[s * segs + g].end());
            want.insert(want.end(), plain[s * segs + g].begin(), plain[s * segs + g].end());
        }
        in_off.push_back(in.size());
        out_off.push_back(want.size());
    }
    uint8_t *d_in = nullptr, *d_out = nullptr;
    uint64_t *d_in_off = nullptr, *d_out_off = nullptr, *d_size = nullptr;
    int32_t *d_status = nullptr;
    HIP_OK(hipMalloc((void **)&d_in, in.size() + 16));
    HIP_OK(hipMalloc((void **)&d_out, want.size() + 16));
    HIP_OK(hipMalloc((void **)&d_in_off, 8 * (streams + 1)));
    HIP_OK(hipMalloc((void **)&d_out_off, 8 * (streams + 1)));
    HIP_OK(hipMalloc((void **)&d_size, 8 * streams));
    HIP_OK(hipMalloc((void **)&d_status, 4 * streams));
    HIP_OK(hipMemcpy(d_in, in.data(), in.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_in_off, in_off.data(), 8 * (streams + 1), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_out_off, out_off.data(), 8 * (streams + 1), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_out, 0xA5, want.size() + 16));
    ez_batch b{};
    b.in = d_in;
    b.in_off = d_in_off;
    b.out = d_out;
    b.out_off = d_out_off;
    b.out_size = d_size;
    b.status = d_status;
    b.count = streams;
    if (DecompressBatchSegmented(0, b, nullptr) != Err::OK) {
        printf("FAIL: the segmented decode\n");
        return 1;
    }
    std::vector<uint8_t> got(want.size() + 16);
    std::vector<uint64_t> size(streams);
    std::vector<int32_t> status(streams);
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(got.data(), d_out, got.size(), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(size.data(), d_size, 8 * streams, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(status.data(), d_status, 4 * streams, hipMemcpyDeviceToHost));
    for (size_t s = 0; s < streams; s++)
        if (status[s] != EZ_OK || size[s] != out_off[s + 1] - out_off[s]) {
            printf("FAIL: stream %zu: status %d size %llu\n", s, status[s], (unsigned long long)size[s]);
            return 1;
        }
    for (size_t k = 0; k < got.size(); k++)
        if (got[k] != (k < want.size() ? want[k] : 0xA5)) {
            printf("FAIL: output byte %zu\n", k);
            return 1;
        }
    uint64_t last[3] = {7, 7, 7};
    if (SegmentsLast(last) != Err::OK || last[0] != streams * segs || last[1] != 0 || last[2] != 0) {
        printf("FAIL: segments %llu, handed over %llu, retries %llu\n", (unsigned long long)last[0], (unsigned long long)last[1],
               (unsigned long long)last[2]);
        return 1;
    }
    bool threw = false;
    try {
        ez_batch bad = b;
        bad.out_size = nullptr;
        (void)DecompressBatchSegmented(0, bad, nullptr);
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    if (!threw) {
        printf("FAIL: a batch without out_size was not refused\n");
        return 1;
    }
    for (void *p : {(void *)d_in, (void *)d_out, (void *)d_in_off, (void *)d_out_off, (void *)d_size, (void *)d_status}) HIP_OK(hipFree(p));
    printf("segments ok\n");
    return 0;
}
