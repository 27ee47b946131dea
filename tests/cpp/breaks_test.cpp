// eazy::StreamBreaksBatch (eazy_amd/cpp/eazy.hpp): 16 streams of 3 to 40 log-like messages of 1 to 4,000
// bytes, each message compressed on its own and joined to its stream with a Break meta behind it (one
// stream starts with a Break, one has two in a row): the query's positions are the running message
// lengths, with and without a workspace, too little room writes none, and the segmented decode's output
// split at the positions gives the messages back.  Needs a device.
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

template <class T>
T *upload(const std::vector<T> &v, size_t extra = 16) {
    T *d = nullptr;
    if (hipMalloc((void **)&d, v.size() * sizeof(T) + extra) != hipSuccess) return nullptr;
    if (!v.empty() && hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return d;
}

}  // namespace

int main() {
    using namespace eazy;
    const size_t streams = 16;
    uint64_t rng = 88172645463325252ull;
    auto rnd = [&]() {
        rng ^= rng << 13;
        rng ^= rng >> 7;
        rng ^= rng << 17;
        return rng;
    };
    // the messages of every stream (an empty one: a Break with nothing before it), compressed in one batch
    std::vector<std::vector<std::vector<uint8_t>>> msgs(streams);
    std::vector<std::vector<uint8_t>> plain, comp;
    for (size_t s = 0; s < streams; s++) {
        const size_t n = 3 + rnd() % 38;
        if (s == 5) msgs[s].push_back({});
        for (size_t k = 0; k < n; k++) {
            msgs[s].push_back(text(1 + rnd() % 4000, (int)(s * 100 + k)));
            if (s == 6 && k == 1) msgs[s].push_back({});
        }
        for (const auto &m : msgs[s])
            if (!m.empty()) plain.push_back(m);
    }
    if (CompressBatchMulti(plain, 1 << 20, 1024, comp, {0}) != Err::OK) {
        printf("FAIL: compress\n");
        return 1;
    }
    std::vector<uint8_t> in, want;
    std::vector<uint64_t> in_off{0}, out_off{0}, idx{0}, pos;
    const Encoder enc{};
    size_t c = 0;
    for (size_t s = 0; s < streams; s++) {
        const size_t o0 = want.size();
        for (const auto &m : msgs[s]) {
            if (!m.empty()) {
                in.insert(in.end(), comp[c].begin(), comp[c].end());
                c++;
                want.insert(want.end(), m.begin(), m.end());
            }
            enc.MetaTag(in, MetaBreak, 0);
            pos.push_back(want.size() - o0);
        }
        in_off.push_back(in.size());
        out_off.push_back(want.size());
        idx.push_back(pos.size());
    }
    const uint64_t found = pos.size();
    uint8_t *d_in = upload(in), *d_out = nullptr;
    uint64_t *d_in_off = upload(in_off), *d_out_off = upload(out_off), *d_size = nullptr, *d_idx = nullptr, *d_pos = nullptr, *d_total = nullptr;
    int32_t *d_status = nullptr;
    void *d_ws = nullptr;
    if (!d_in || !d_in_off || !d_out_off) {
        printf("FAIL: upload\n");
        return 1;
    }
    HIP_OK(hipMalloc((void **)&d_out, want.size() + 16));
    HIP_OK(hipMalloc((void **)&d_size, 8 * streams));
    HIP_OK(hipMalloc((void **)&d_status, 4 * streams));
    HIP_OK(hipMalloc((void **)&d_idx, 8 * (streams + 1)));
    HIP_OK(hipMalloc((void **)&d_pos, 8 * (found + 1)));
    HIP_OK(hipMalloc((void **)&d_total, 16));
    HIP_OK(hipMalloc(&d_ws, ez_breaks_workspace(streams)));
    HIP_OK(hipMemset(d_ws, 0xA5, ez_breaks_workspace(streams)));
    ez_batch b{};
    b.in = d_in;
    b.in_off = d_in_off;
    b.out_size = d_size;
    b.status = d_status;
    b.count = streams;
    std::vector<uint64_t> g_idx(streams + 1), g_pos(found + 1), g_size(streams);
    std::vector<int32_t> g_status(streams);
    uint64_t total[2];
    for (int round = 0; round < 3; round++) {  // with a workspace, without one, with too little room
        const uint64_t cap = round == 2 ? found - 1 : found;
        HIP_OK(hipMemset(d_pos, 0xA5, 8 * (found + 1)));
        if (StreamBreaksBatch(0, b, d_idx, d_pos, cap, d_total, round == 1 ? nullptr : d_ws, nullptr) != Err::OK) {
            printf("FAIL: the break query, round %d\n", round);
            return 1;
        }
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(g_idx.data(), d_idx, 8 * (streams + 1), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(g_pos.data(), d_pos, 8 * (found + 1), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(g_size.data(), d_size, 8 * streams, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(g_status.data(), d_status, 4 * streams, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(total, d_total, 16, hipMemcpyDeviceToHost));
        if (total[1] != found || total[0] != (round == 2 ? 0 : found) || g_idx != idx) {
            printf("FAIL: round %d: brk_total {%llu, %llu}, %llu Breaks built\n", round, (unsigned long long)total[0], (unsigned long long)total[1],
                   (unsigned long long)found);
            return 1;
        }
        for (size_t s = 0; s < streams; s++)
            if (g_status[s] != EZ_OK || g_size[s] != out_off[s + 1] - out_off[s]) {
                printf("FAIL: round %d, stream %zu: status %d size %llu\n", round, s, g_status[s], (unsigned long long)g_size[s]);
                return 1;
            }
        for (size_t k = 0; k <= found; k++)
            if (g_pos[k] != (k < found && round != 2 ? pos[k] : 0xA5A5A5A5A5A5A5A5ull)) {
                printf("FAIL: round %d: brk_pos[%zu] = %llu\n", round, k, (unsigned long long)g_pos[k]);
                return 1;
            }
    }
    // the recipe: decode, then split every stream's output at its Breaks
    b.out = d_out;
    b.out_off = d_out_off;
    if (DecompressBatchSegmented(0, b, nullptr) != Err::OK) {
        printf("FAIL: the segmented decode\n");
        return 1;
    }
    std::vector<uint8_t> got(want.size());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(got.data(), d_out, got.size(), hipMemcpyDeviceToHost));
    for (size_t s = 0; s < streams; s++) {
        uint64_t from = 0;
        for (size_t k = 0; k < msgs[s].size(); k++) {
            const uint64_t to = pos[idx[s] + k];
            const std::vector<uint8_t> m(got.begin() + (ptrdiff_t)(out_off[s] + from), got.begin() + (ptrdiff_t)(out_off[s] + to));
            if (m != msgs[s][k]) {
                printf("FAIL: stream %zu, message %zu\n", s, k);
                return 1;
            }
            from = to;
        }
    }
    bool threw = false;
    try {
        (void)StreamBreaksBatch(0, b, d_idx, nullptr, 4, d_total, d_ws, nullptr);
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    if (!threw) {
        printf("FAIL: a null brk_pos with room was not refused\n");
        return 1;
    }
    for (void *p : {(void *)d_in, (void *)d_out, (void *)d_in_off, (void *)d_out_off, (void *)d_size, (void *)d_status, (void *)d_idx, (void *)d_pos,
                    (void *)d_total, d_ws})
        HIP_OK(hipFree(p));
    printf("breaks ok\n");
    return 0;
}
