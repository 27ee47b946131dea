// eazy::DecompressedSizeBatchMulti (eazy_amd/cpp/eazy.hpp) against the streams' known lengths and
// against DecompressBatchMulti: a ragged batch with empty streams and a truncated one, over one
// shard and over two shards of device 0; the sizes then lay out the decode's slots.  Needs a device.
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

}  // namespace

int main() {
    using namespace eazy;
    const size_t lens[] = {100000, 0, 7, 400000, 0, 65536, 1, 250001};
    std::vector<std::vector<uint8_t>> plain, comp;
    for (size_t k = 0; k < sizeof lens / sizeof lens[0]; k++) plain.push_back(text(lens[k], (int)k));
    if (CompressBatchMulti(plain, 1 << 20, 1024, comp, {0}) != Err::OK) {
        printf("FAIL: compress\n");
        return 1;
    }
    std::vector<std::vector<uint8_t>> streams = comp;
    streams.push_back(std::vector<uint8_t>(comp[3].begin(), comp[3].end() - 5));  // truncated
    streams.push_back({});                                                         // no bytes at all
    for (const std::vector<int> &devs : {std::vector<int>{0}, std::vector<int>{0, 0}}) {
        std::vector<std::pair<uint64_t, Err>> got;
        if (DecompressedSizeBatchMulti(streams, got, devs) != Err::OK || got.size() != streams.size()) {
            printf("FAIL: the query over %zu shard(s)\n", devs.size());
            return 1;
        }
        for (size_t k = 0; k < plain.size(); k++)
            if (got[k].first != plain[k].size() || got[k].second != Err::OK) {
                printf("FAIL: stream %zu over %zu shard(s): size %llu status %d\n", k, devs.size(), (unsigned long long)got[k].first, (int)got[k].second);
                return 1;
            }
        const size_t t = plain.size();
        if (got[t].second == Err::OK || got[t].first >= plain[3].size() || got[t + 1].first != 0 || got[t + 1].second != Err::OK) {
            printf("FAIL: the truncated or the empty stream over %zu shard(s)\n", devs.size());
            return 1;
        }
        // the decode into slots of exactly those sizes: the same sizes and statuses, the plain bytes
        std::vector<uint64_t> slots;
        for (const auto &g : got) slots.push_back((g.first + 15) & ~(uint64_t)15);
        std::vector<std::pair<std::vector<uint8_t>, Err>> dec;
        if (DecompressBatchMulti(streams, slots, dec, devs) != Err::OK) {
            printf("FAIL: the decode over %zu shard(s)\n", devs.size());
            return 1;
        }
        for (size_t k = 0; k < streams.size(); k++)
            if (dec[k].first.size() != got[k].first || dec[k].second != got[k].second || (k < plain.size() && dec[k].first != plain[k])) {
                printf("FAIL: stream %zu decoded differs from the query\n", k);
                return 1;
            }
    }
    if (ez_decompressed_size_batch_multi(0, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr) != EZ_EINVAL) {
        printf("FAIL: NULL in_off and out_size were not refused\n");
        return 1;
    }
    printf("size_multi ok\n");
    return 0;
}
