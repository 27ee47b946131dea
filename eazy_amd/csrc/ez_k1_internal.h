// ez_k1_internal.h — host interface between the K1 translation units: the routing
// (ez_compress_split.hip) and the kernel families' launchers (ez_k1_parse.hip, ez_k1_lean.hip,
// ez_k1_long.hip, ez_k1_chunk.hip, ez_k1_emit.hip, ez_k1_probe.hip).  ez_internal.h stays the
// interface between the C-ABI and the kernels.
#pragma once

#include "ez_k1_device.h"

namespace ez {

// LDS words of a stream's table (0 = this variant cannot take the batch)
template <bool T16>
uint32_t split_table_words(const CompressArgs &a) {
    if (a.ring || a.max_len == 0 || 2 * (int64_t)a.max_len > a.bs || a.hs > 4096 || a.hs < 4) return 0;
    if ((int64_t)a.max_len > (T16 ? k1::kMaxT16 : k1::kMaxT32)) return 0;
    const uint64_t words = T16 ? ((uint64_t)a.hs + 1) / 2 : (uint64_t)a.hs;
    return (uint32_t)((words + 3) & ~3ull);
}
template <int G, bool T16>
uint32_t split_stride(const CompressArgs &a) {
    const uint64_t tw = split_table_words<T16>(a);
    if (tw == 0) return 0;
    const uint64_t w = tw;
    if (w * 4 * (64 / G) > 160 * 1024) return 0;
    return (uint32_t)w;
}
inline uint64_t up256(uint64_t x) { return (x + 255) & ~255ull; }

// ez_k1_parse.hip: k1_parse + the token writer; instantiated for (16, true, MW), (16, false, MW)
// and (32, false, MW)
template <int G, bool T16, bool MW>
hipError_t launch_split_g(const CompressArgs &a, uint64_t *recs, hipStream_t st);
// ez_k1_lean.hip: k1_lean + the token writer (single-Write batches on the u16 table)
hipError_t launch_lean(const CompressArgs &a, uint64_t *recs, hipStream_t st);
// ez_k1_long.hip: the k1_long launch alone, S streams per wave; only / ostride: K1c's fail words
// (k1_long's `only`), nullptr for every stream
hipError_t launch_k1_long(const CompressArgs &a, uint4 *recs, uint64_t rcap, uint32_t S, const uint32_t *only, uint32_t ostride,
                          hipStream_t st);
// ez_k1_chunk.hip: K1c on K1L's scratch (launch_long takes it when chunk_applies), and its
// workspace's bytes after the records and the token writer's workspace
hipError_t launch_chunk(const CompressArgs &a, uint8_t *recs, hipStream_t st);
uint64_t chunk_scratch_bytes(const CompressArgs &a);
// ez_k1_emit.hip: the token writer, one wave per stream (k1_emit<WIDE>; WIDE: 16-byte records), and
// for 16-byte records the choice between it and the chip-wide ke_size / ke_scan / ke_write with
// their workspace ws of ew_bytes
hipError_t launch_emit(const CompressArgs &a, const uint64_t *recs, uint64_t rcap, bool wide_recs, hipStream_t st);
uint64_t ew_bytes(const CompressArgs &a);
hipError_t launch_emit_wide(const CompressArgs &a, const uint4 *recs, uint64_t rcap, uint8_t *ws, hipStream_t st);
// ez_k1_probe.hip: same-address LDS stores of one wave instruction land in ascending lane order
// (u16: T16's table; u32: K1L's); the other probes are the C-ABI's too (ez_internal.h)
bool lds_store_in_lane_order();
bool lds_store32_in_lane_order();

}  // namespace ez
