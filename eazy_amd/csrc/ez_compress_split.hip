// ez_compress_split.hip — K1s routing: which kernel family a batch of fresh streams takes, and
// the scratch it needs.  The families: ez_k1_parse.hip (k1_parse), ez_k1_lean.hip (k1_lean),
// ez_k1_long.hip (K1L), ez_k1_chunk.hip (K1c), ez_k1_emit.hip (the token writers);
// ez_k1_probe.hip checks the LDS properties the choice rests on.
#include "ez_k1_internal.h"

#include <atomic>

namespace ez {
namespace {
using namespace k1;

// lanes per stream for T32: 32 when the batch has few streams (long Writes, C2: two
// waves per SIMD instead of one, 33.3 vs 34.3 ms); EZ_K1S_G32=16|32 overrides
int split_g32(uint64_t count) {
    static const int g = knob("EZ_K1S_G32", 0);
    if (g == 32 || g == 16) return g;
    return count <= 8192 ? 32 : 16;
}
std::atomic<bool> g_split_t32{false};  // ez_select_compress_kernel('S')
bool split_t32_forced() {
    static const bool v = knob("EZ_K1S_T", 0) == 32;
    return v || g_split_t32;
}

// the table the batch takes: 16 (T16), 32 (T32) or 0 (K1s cannot take it)
int split_table(const CompressArgs &a) {
    if (a.count > (1ull << 31)) return 0;
    if (!split_t32_forced() && split_stride<16, true>(a) != 0 && lds_store_in_lane_order()) return 16;
    if (split_stride<16, false>(a) != 0 && lds_exchange_in_lane_order()) return 32;
    return 0;
}

bool split_takes_long(const CompressArgs &a) {
    return !a.write_idx && !split_t32_forced() && split_table(a) != 16 && long_applies(a);
}

}  // namespace

void select_split_table(bool t32) { g_split_t32 = t32; }

bool split_applies(const CompressArgs &a) { return split_table(a) != 0; }

// K1L's scratch, or records (8 bytes per record slot entry), then k1_lean's edge area
uint64_t split_scratch_words(const CompressArgs &a) {
    if (split_takes_long(a)) return (long_scratch_bytes(a) + 3) / 4;
    return a.count * rec_cap(a) * 2 + (edge_area_bytes(a) + 3) / 4;
}

// K1s routing: one Write per stream on the u16 table -> k1_lean (k1_parse on a device whose
// ds_mskor probe fails); one Write per stream on the u32 table (streams over 64 KiB) -> K1L;
// multi-Write streams and forced T32 -> k1_parse, 32 lanes per stream for batches of few streams
hipError_t launch_compress_split(const CompressArgs &a, uint32_t *scratch, hipStream_t st) {
    uint64_t *recs = (uint64_t *)scratch;
    const int T = split_table(a);
    if (a.write_idx) {
        if (T == 16) return launch_split_g<16, true, true>(a, recs, st);
        if (split_g32(a.count) == 32) return launch_split_g<32, false, true>(a, recs, st);
        return launch_split_g<16, false, true>(a, recs, st);
    }
    if (T == 16) return lds_mskor_in_lane_order() ? launch_lean(a, recs, st) : launch_split_g<16, true, false>(a, recs, st);
    // single Writes on the u32 table (streams over 64 KiB, C2): K1L, the lean parse (C2 31.5 vs 33.7 ms)
    if (split_takes_long(a)) return launch_long(a, (uint8_t *)scratch, st);
    if (split_g32(a.count) == 32) return launch_split_g<32, false, false>(a, recs, st);
    return launch_split_g<16, false, false>(a, recs, st);
}

}  // namespace ez
