// Host check of the size query's K2g stage (k2g_size, eazy_amd/csrc/ez_decompress_segs.hip): the
// per-lane steps of ez_k2_segs.h and its end step kg_end_ok, compiled for the CPU and run over 64
// emulated lanes as the kernel runs them (the wave's walk of a super-block, kg_sum, the events in lane
// order through kg_cuts with a cut that stores nothing, then kg_end_ok), for every chunk size.
//   k2_segs_size_check F    F: the streams tools/k2_segs_check --dump wrote
// To the dumped streams it adds one of them that has several cuts, truncated at each of its last 27
// bytes, and four of its own whose last segment fails the end check (no dumped stream does: an error
// before the last segment stops the walk at the next Reset).  Per stream and chunk size:
//   the verdict (sized, or handed on) and, where sized, the total equal a single walker's (kg_serial
//   and kg_end_ok);
//   a sized stream's total is the output length of the oracle's Reader read to EOF, which ends
//   without an error;
//   a dumped stream with a cut, no stop and no error from the oracle is sized.
// Prints the count of every class, exits 1 at the first mismatch.
#include "../eazy_amd/csrc/ez_k2_segs.h"
#include "k2_check_common.h"

using namespace k2check;

namespace {

struct Counts {
    uint64_t streams, dumped, sized, sized_with_cuts, handed_stop, handed_end, truncations, truncations_sized, own, must_size, superblocks,
        events, chunk64, chunk256, chunk1024;
} N;

struct Verdict {
    bool sized, stop;
    uint64_t total;
    uint32_t ncut;
};

Verdict verdict(const ez::KgState &st, uint32_t end, uint32_t nb) { return Verdict{ez::kg_end_ok(st, end, nb), st.stop, st.total, st.ncut}; }

// the kernel's loop over a stream, 64 lanes emulated in order
template <int C>
Verdict emulate(const Bytes &s, int64_t limit) {
    using namespace ez;
    const int32_t lim32 = k2_lim32(limit);
    const uint32_t nb = (uint32_t)s.size();
    auto cut = [](uint32_t, uint32_t, uint64_t) {};
    KgState st = kg_start();
    uint32_t sb = 0;
    EmuWave<C> wv(kz_stage_bytes(C));
    EmuStats es{};
    while (!st.stop && sb < nb) {
        N.superblocks++;
        const KzWin w = emu_walk<C>(wv, s.data(), nb, sb, sb, true, sb, es);
        if (!wv.settled) {
            st.stop = true;
            break;
        }
        KgSum r[kZLanes];
        for (int l = 0; l < kZLanes; l++) r[l] = kg_sum<C>(w, sb, l, nb, wv.a[l], wv.x[l], lim32, limit);
        for (int l = 0; l < kZLanes && !st.stop; l++) {  // (the kernel: the prefix up to each event, then kg_cuts on every lane)
            st.total += r[l].out;
            st.maxd = r[l].maxd > st.maxd ? r[l].maxd : st.maxd;
            if (r[l].fl == 0) continue;
            N.events++;
            kg_cuts<C>(w, sb, l, nb, r[l].epos, wv.x[l], lim32, limit, st, cut);
        }
        if (st.stop) break;
        sb = wv.x[kZLanes - 1];
    }
    return verdict(st, sb, nb);
}

Verdict serial(const Bytes &s, int64_t limit) {
    const Padded at(s);
    uint32_t end = 0;
    const ez::KgState st = ez::kg_serial([&](uint32_t p) { return at(p); }, (uint32_t)s.size(), ez::k2_lim32(limit), limit,
                                         [](uint32_t, uint32_t, uint64_t) {}, &end);
    return verdict(st, end, (uint32_t)s.size());
}

// one stream: the three chunked walks against the serial one, a sized one against the oracle; returns
// the verdict.  must: the dump says it has a cut and no stop (then sized, unless the oracle reports an error)
Verdict check_one(const std::string &name, const Bytes &s, int64_t limit, bool must) {
    const Verdict one = serial(s, limit);
    for (int c = 0; c < 3; c++) {
        const Verdict r = c == 0 ? emulate<64>(s, limit) : (c == 1 ? emulate<256>(s, limit) : emulate<1024>(s, limit));
        (c == 0 ? N.chunk64 : (c == 1 ? N.chunk256 : N.chunk1024))++;
        if (r.sized != one.sized || r.stop != one.stop || (r.sized && r.total != one.total)) {
            std::printf("MISMATCH %s (%zu bytes, chunk %d): serial walk sized %d stop %d total %llu | the stage sized %d stop %d total %llu\n",
                        name.c_str(), s.size(), c == 0 ? 64 : (c == 1 ? 256 : 1024), (int)one.sized, (int)one.stop, (unsigned long long)one.total,
                        (int)r.sized, (int)r.stop, (unsigned long long)r.total);
            std::exit(1);
        }
    }
    int64_t olen = 0;
    const int err = oracle(s.data(), s.size(), limit, olen);
    if (one.sized && (err != 0 || (uint64_t)olen != one.total)) {
        std::printf("MISMATCH %s (%zu bytes): sized as %llu bytes and OK, the oracle reads %lld bytes and ends with %d\n", name.c_str(), s.size(),
                    (unsigned long long)one.total, (long long)olen, err);
        std::exit(1);
    }
    if (must && err == 0) {
        N.must_size++;
        if (!one.sized) {
            std::printf("MISMATCH %s (%zu bytes): a stream with a cut, no stop and no error is handed on (stop %d)\n", name.c_str(), s.size(),
                        (int)one.stop);
            std::exit(1);
        }
    }
    N.streams++;
    if (one.sized) N.sized++;
    if (one.sized && one.ncut) N.sized_with_cuts++;
    if (!one.sized) (one.stop ? N.handed_stop : N.handed_end)++;
    return one;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    g_out.resize(16 << 20);
    Bytes multi;  // the first dumped stream with at least 3 cuts, no stop and no BlockSizeLimit
    for (;;) {
        uint64_t h[5];
        if (std::fread(h, 8, 5, f) != 5) break;
        std::string name(h[0], ' ');
        Bytes s(h[2]);
        std::vector<uint64_t> cuts(2 * h[3]);
        if (std::fread(&name[0], 1, name.size(), f) != name.size() || std::fread(s.data(), 1, s.size(), f) != s.size() ||
            std::fread(cuts.data(), 8, cuts.size(), f) != cuts.size()) {
            std::printf("the dump ends inside a stream\n");
            return 2;
        }
        N.dumped++;
        check_one(name, s, (int64_t)h[1], h[3] >= 1 && h[4] == 0);
        if (multi.empty() && h[3] >= 3 && h[4] == 0 && h[1] == 0) multi = s;
    }
    std::fclose(f);
    if (multi.empty()) {
        std::printf("the dump holds no stream with 3 cuts\n");
        return 2;
    }
    for (size_t cut = 1; cut <= 27 && cut <= multi.size(); cut++) {
        N.truncations++;
        if (check_one("multi-cut stream cut " + std::to_string(cut), Bytes(multi.begin(), multi.end() - (long)cut), 0, false).sized)
            N.truncations_sized++;
    }
    {  // a last segment that fails the end check: nothing after it stops the walk
        Bytes a;  // a distance past its own segment's window (ErrOverflow), the segment before has none
        hdr(a, 20);
        fill_to(a, 300);
        rst(a, 10);
        lit_rnd(a, 50);
        cpy(a, 5000, 40);
        Bytes b;  // the same in a stream's only segment
        hdr(b, 10);
        lit_rnd(b, 50);
        cpy(b, 5000, 40);
        Bytes c;  // output without any window
        lit_rnd(c, 7);
        Bytes d = multi;  // several good cuts, then the distance
        rst(d, 10);
        lit_rnd(d, 9);
        cpy(d, 1025, 4);
        const Bytes *own[4] = {&a, &b, &c, &d};
        for (int k = 0; k < 4; k++) {
            N.own++;
            const Verdict v = check_one("own stream " + std::to_string(k), *own[k], 0, false);
            if (v.sized || v.stop) {
                std::printf("MISMATCH own stream %d: built to fail the end check, sized %d stop %d\n", k, (int)v.sized, (int)v.stop);
                return 1;
            }
        }
    }
#define P(f) K2_COUNT(N, 20, f)
    P(streams); P(dumped); P(sized); P(sized_with_cuts); P(handed_stop); P(handed_end); P(truncations); P(truncations_sized); P(own);
    P(must_size); P(superblocks); P(events); P(chunk64); P(chunk256); P(chunk1024);
    std::printf("ok\n");
    return 0;
}
