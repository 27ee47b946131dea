// eazy::WriteMany (eazy_amd/cpp/eazy.hpp) against Writer::Write: 4 Writers with recording sinks, one
// with a FlushThreshold and one without the magic, three rounds of one line each.  Needs a device.
#include <cstdio>
#include <string>
#include <string_view>
#include <vector>

#include "../../eazy_amd/cpp/eazy.hpp"

namespace {

struct Sink : eazy::IoWriter {
    std::vector<std::string> calls;
    std::pair<size_t, eazy::Err> Write(const uint8_t *p, size_t n) override {
        calls.emplace_back((const char *)p, n);
        return {n, eazy::Err::OK};
    }
};

std::string line(int round, int j) {
    std::string s = "2026-01-01T00:00:0" + std::to_string(round) + " INFO tenant-" + std::to_string(j) + " GET /api/v1/items/";
    for (int k = 0; k < 3 + j; k++) s += std::to_string(1000 * round + 37 * j + k) + " status=200 ";
    return s;
}

std::vector<std::vector<std::string>> run(bool many) {
    constexpr int N = 4, ROUNDS = 3;
    Sink sinks[N];
    std::vector<std::unique_ptr<eazy::Writer>> own;
    std::vector<eazy::Writer *> ws;
    for (int j = 0; j < N; j++) {
        own.push_back(eazy::NewWriter(&sinks[j], j % 2 ? 1024 : 65536, j % 2 ? 256 : 1024));
        ws.push_back(own.back().get());
    }
    ws[1]->FlushThreshold = 96;
    ws[2]->AppendMagic = false;
    for (int r = 0; r < ROUNDS; r++) {
        std::vector<std::string> ls;
        for (int j = 0; j < N; j++) ls.push_back(line(r, j));
        if (many) {
            std::vector<std::string_view> ps(ls.begin(), ls.end());
            auto [took, err] = eazy::WriteMany(ws, ps);
            if (err != eazy::Err::OK) return {};
            for (int j = 0; j < N; j++)
                if (took[j] != ls[j].size()) return {};
        } else {
            for (int j = 0; j < N; j++)
                if (ws[j]->Write(ls[j]).second != eazy::Err::OK) return {};
        }
    }
    std::vector<std::vector<std::string>> out;
    for (int j = 0; j < N; j++) {
        if (ws[j]->Flush() != eazy::Err::OK) return {};
        out.push_back(sinks[j].calls);
    }
    return out;
}

}  // namespace

int main() {
    const auto a = run(true), b = run(false);
    if (a.size() != 4 || b.size() != 4) {
        printf("FAIL: a call failed\n");
        return 1;
    }
    for (size_t j = 0; j < 4; j++) {
        if (a[j] != b[j] || a[j].empty()) {
            printf("FAIL: Writer %zu: WriteMany's sink calls differ from Write's\n", j);
            return 1;
        }
    }
    uint64_t counts[2] = {0, 0};
    ez_writer_write_many_last(counts);
    if (counts[0] != 4 || counts[1] != 0) {
        printf("FAIL: %llu Writes in the launch, %llu on their own path\n", (unsigned long long)counts[0], (unsigned long long)counts[1]);
        return 1;
    }
    printf("write_many ok\n");
    return 0;
}
