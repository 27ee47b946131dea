// eazy::DecompressBatchSized (eazy_amd/cpp/eazy.hpp): streams whose decoded lengths are unknown, sized
// with DecompressedSizeBatch and decoded into slots laid out from its answer.  64 streams of 4
// compressed streams joined back to back: the size query's K2g stage sizes all 64, the decode is the
// segmented one (256 segments) and the plain bytes come back.  Then the 256 streams on their own: the
// stage sees nothing, and the decode is DecompressBatch's on a fast decoder.  Needs a device.
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

#define HIP_OK(x)                     \
    do {                              \
        if ((x) != hipSuccess) {      \
            printf("FAIL: %s\n", #x); \
            return 1;                 \
        }                             \
    } while (0)

// sizes, lays out slots of the sizes rounded up to 16 bytes, decodes, compares with want (the streams'
// plain bytes in order); joined: the streams the stage must have sized
int round_trip(const std::vector<std::vector<uint8_t>> &streams, const std::vector<std::vector<uint8_t>> &want, uint64_t joined) {
    using namespace eazy;
    const size_t count = streams.size();
    std::vector<uint8_t> in;
    std::vector<uint64_t> in_off{0};
    for (const auto &s : streams) {
        in.insert(in.end(), s.begin(), s.end());
        in_off.push_back(in.size());
    }
    uint8_t *d_in = nullptr, *d_out = nullptr;
    uint64_t *d_in_off = nullptr, *d_out_off = nullptr, *d_size = nullptr;
    int32_t *d_status = nullptr;
    void *d_ws = nullptr;
    HIP_OK(hipMalloc((void **)&d_in, in.size() + 16));
    HIP_OK(hipMalloc((void **)&d_in_off, 8 * (count + 1)));
    HIP_OK(hipMalloc((void **)&d_out_off, 8 * (count + 1)));
    HIP_OK(hipMalloc((void **)&d_size, 8 * count));
    HIP_OK(hipMalloc((void **)&d_status, 4 * count));
    HIP_OK(hipMalloc(&d_ws, ez_decompress_workspace(count)));
    HIP_OK(hipMemcpy(d_in, in.data(), in.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_in_off, in_off.data(), 8 * (count + 1), hipMemcpyHostToDevice));
    ez_batch b{};
    b.in = d_in;
    b.in_off = d_in_off;
    b.out_size = d_size;
    b.status = d_status;
    b.count = count;
    if (DecompressedSizeBatch(0, b, d_ws, nullptr) != Err::OK) {
        printf("FAIL: the size query\n");
        return 1;
    }
    HIP_OK(hipDeviceSynchronize());
    std::vector<uint64_t> size(count), out_off{0};
    std::vector<int32_t> status(count);
    HIP_OK(hipMemcpy(size.data(), d_size, 8 * count, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(status.data(), d_status, 4 * count, hipMemcpyDeviceToHost));
    for (size_t s = 0; s < count; s++) {
        if (status[s] != EZ_OK || size[s] != want[s].size()) {
            printf("FAIL: stream %zu sized: status %d size %llu\n", s, status[s], (unsigned long long)size[s]);
            return 1;
        }
        out_off.push_back(out_off.back() + ((size[s] + 15) & ~(uint64_t)15));
    }
    uint64_t c[3] = {7, 7, 7};
    if (DecompressedSizeSegsLast(d_ws, count, c) != Err::OK || c[0] != joined || c[1] != joined || c[2] != 0) {
        printf("FAIL: the stage took %llu, sized %llu, handed on %llu\n", (unsigned long long)c[0], (unsigned long long)c[1],
               (unsigned long long)c[2]);
        return 1;
    }
    uint64_t before[3] = {0, 0, 0}, after[3] = {0, 0, 0};
    if (SegmentsLast(before) != Err::OK) return 1;
    HIP_OK(hipMalloc((void **)&d_out, out_off.back() + 16));
    HIP_OK(hipMemset(d_out, 0xA5, out_off.back() + 16));
    HIP_OK(hipMemcpy(d_out_off, out_off.data(), 8 * (count + 1), hipMemcpyHostToDevice));
    b.out = d_out;
    b.out_off = d_out_off;
    if (DecompressBatchSized(0, b, d_ws, nullptr) != Err::OK) {
        printf("FAIL: the sized decode\n");
        return 1;
    }
    HIP_OK(hipDeviceSynchronize());
    std::vector<uint8_t> got(out_off.back() + 16);
    HIP_OK(hipMemcpy(got.data(), d_out, got.size(), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(size.data(), d_size, 8 * count, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(status.data(), d_status, 4 * count, hipMemcpyDeviceToHost));
    for (size_t s = 0; s < count; s++) {
        if (status[s] != EZ_OK || size[s] != want[s].size()) {
            printf("FAIL: stream %zu decoded: status %d size %llu\n", s, status[s], (unsigned long long)size[s]);
            return 1;
        }
        for (uint64_t k = out_off[s]; k < out_off[s + 1]; k++)
            if (got[k] != (k - out_off[s] < size[s] ? want[s][k - out_off[s]] : 0xA5)) {
                printf("FAIL: stream %zu, output byte %llu\n", s, (unsigned long long)(k - out_off[s]));
                return 1;
            }
    }
    if (SegmentsLast(after) != Err::OK) return 1;
    if (joined ? after[0] != 4 * joined : (after[0] != before[0] || ez_decompress_kernel_last() == 'e')) {
        printf("FAIL: %llu streams sized by the stage, segments_last %llu -> %llu, first decoder %c\n", (unsigned long long)joined,
               (unsigned long long)before[0], (unsigned long long)after[0], ez_decompress_kernel_last());
        return 1;
    }
    for (void *p : {(void *)d_in, (void *)d_out, (void *)d_in_off, (void *)d_out_off, (void *)d_size, (void *)d_status, d_ws}) HIP_OK(hipFree(p));
    return 0;
}

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
    std::vector<std::vector<uint8_t>> joined(streams), want(streams);
    for (size_t s = 0; s < streams; s++)
        for (size_t g = 0; g < segs; g++) {
            joined[s].insert(joined[s].end(), comp[s * segs + g].begin(), comp[s * segs + g].end());
            want[s].insert(want[s].end(), plain[s * segs + g].begin(), plain[s * segs + g].end());
        }
    if (round_trip(joined, want, streams)) return 1;
    if (round_trip(comp, plain, 0)) return 1;
    bool threw = false;
    try {
        uint64_t c[3];
        (void)DecompressedSizeSegsLast(nullptr, 4, c);
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    if (!threw) {
        printf("FAIL: a NULL workspace was not refused\n");
        return 1;
    }
    printf("sized ok\n");
    return 0;
}
