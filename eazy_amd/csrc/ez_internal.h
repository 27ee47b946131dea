// ez_internal.h — launch interface between the C-ABI (ez_capi.hip and its handle files) and the
// gfx950 kernels (ez_compress.hip, ez_decompress.hip, ez_pack.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ez {

// Timing / A-B switches.  Only experiment builds (make exp: -DEZ_KNOBS) read them from the
// environment; the product library reads no environment and runs the defaults (kernel choices for
// tests go through ez_select_compress_kernel / ez_select_decompress_kernel).
#ifdef EZ_KNOBS
const char *knob_str(const char *name);
int knob(const char *name, int dflt);
#else
inline const char *knob_str(const char *) { return nullptr; }
inline int knob(const char *, int dflt) { return dflt; }
#endif

// K1x per-stream state (ez_compress_spec.hip): speculation restarts at `from`, the pending literal
// starts at `done`, the stream's output so far is `op` bytes; flags: 0 active, 1 finished
struct SpecState {
    uint32_t from, done, op, flags;
};
// K2t, K2w: a long literal kd_copy moves after the decoders (len bytes from in[src] to out[dst])
struct DeferLit {
    uint64_t src, dst, len;
};
constexpr int kDefSlots = 8;  // deferred literals per stream at most
// a literal whose bytes K1x copies at the end (kx_copy): len bytes from in[src] to out[dst]
struct SpecLit {
    uint64_t src, dst, len;
};

// One K1 launch: `count` independent streams (batch) or one stream of a
// writer handle (ring != nullptr, ht_global persistent).
struct CompressArgs {
    const uint8_t *in;
    const uint64_t *in_off;   // count+1
    uint8_t *out;
    const uint64_t *out_off;  // count+1 (slot capacities)
    uint64_t *out_size;       // count
    int32_t *status;          // count or nullptr
    uint64_t count;
    int64_t bs;               // block (window) size, power of two
    int64_t hs;               // hash-table entries, power of two
    int append_magic;
    int ver;
    int header;               // emit the stream header first (isreset)
    // writer-handle mode
    int64_t start;            // stream position of in[0] (w.pos at Write entry)
    uint8_t *ring;            // the handle's ring (block), updated in place; nullptr = fresh stream
    uint32_t *ht_global;      // persistent hash table (handle) / per-block scratch (large hs)
    uint64_t max_len;         // max stream length (0 = unknown)
    // batch of multi-Write streams (nullptr = one Write per stream): stream s receives
    // the Writes k = write_idx[s] .. write_idx[s+1]-1, Write k ending at in[write_end[k]]
    const uint64_t *write_idx;
    const uint64_t *write_end;
    uint64_t max_writes;      // the most Writes of one stream (records reserved for their ends)
    uint64_t *write_out;      // general kernel: the output size after each Write (nullptr: not recorded)
    // K1x rounds (ez_compress_spec.hip): the general kernel resumes a stream from K1x's state
    //   spec_mode 1: at spec_first[s] (streams with ~0u there are skipped), with the table
    //                spec_tab[s]; stops after the first accepted copy and stores its state back;
    //                its literals' bytes are left to kx_copy (a record in spec_lit each)
    //   spec_mode 2: at spec[s].from, to the end of the stream
    // streams whose spec[s].flags != 0 are finished and skipped
    int spec_mode;
    SpecState *spec;
    const uint32_t *spec_first;
    uint32_t *spec_tab;
    SpecLit *spec_lit;
    uint32_t *spec_nlit;
    uint32_t win_bytes;       // general kernel, long streams: LDS window bytes (set by its launcher)
    int no_k1c;               // K1c's workspace could not be had: K1L alone (set by the C-ABI's retry)
    // a Writer handle's Write on K1L's LDS path: when set, the kernel's last act is storing done_seq
    // there (pinned host memory, system scope) so that the caller can wait by polling it
    uint32_t *done_flag;
    uint32_t done_seq;
};


// One K2 launch.  Batch: count complete streams from fresh Readers.
// Handle: count == 1 with the streaming state in `st`.
struct DecodeState {
    int64_t bs;       // len(r.block) (0 = no MetaReset seen yet)
    int64_t pos;      // r.pos
    int64_t off;      // r.off (absolute)
    int64_t len;      // r.len
    int32_t state;    // 0, 'l', 'c'
    int32_t ver;      // r.d.Ver
    int64_t i;        // r.i (in / out)
    int64_t n;        // bytes produced (out)
    int64_t detail;   // meta id / version of the last error
    int64_t hist;     // bytes of the current block held before out (handle mode)
    int32_t err;      // result code
    int32_t pad;
};

struct DecompressArgs {
    const uint8_t *in;
    const uint64_t *in_off;   // count+1
    uint8_t *out;
    const uint64_t *out_off;  // count+1 (capacities)
    uint64_t *out_size;       // count
    int32_t *status;          // count or nullptr
    uint64_t count;
    int64_t block_size_limit;
    int require_magic;
    int skip_unsupported_meta;
    int handle;               // 1 = single streaming call (Reader.Read loop without refill)
    int more;                 // handle: in is a window of the Reader's buffer, which goes on after it (see d_continue_meta)
    int64_t boff;             // handle: absolute offset of in[0]
    DecodeState *st;          // handle: state in/out
    uint32_t *slow;           // batch: [0] = count, [1..] = streams the fast path handed over (nullptr = exact path only)
    uint32_t *defer;          // K2t, K2w: [0] = count, records (DeferLit) from word 4: long literals kd_copy moves
    uint64_t defer_cap;       // records reserved
    uint64_t max_out;         // batch: host hint, largest output slot (0 = unknown)
    const uint32_t *todo;     // batch: [0] = count, [1..] = the streams to decode (nullptr = all)
    // one-stream batches (count == 1, a Reader handle's whole-stream decode), optional, K2t and the exact
    // decoder: breaks[0] counts the Break metas the decoders skip (reader.go:306-307) and breaks[1 ..
    // breaks_cap] get their output positions (unordered); end_state gets {len(r.block), r.pos} at the end
    // of the stream (the Reader's state after the last token, for a Read-by-Read continuation)
    uint64_t *breaks;
    uint64_t breaks_cap;
    int64_t *end_state;
    // K2j's workspace, optional (jump_workspace_bytes): a synchronous caller (a Reader handle) passes
    // one it owns; without it the launcher keeps one per (device, HIP stream).  The size query takes
    // the parts route's scratch the same way (size_parts_workspace_bytes)
    void *jws;
    uint64_t jws_cap;
    int force;                // batch: the first K2 kernel ('r', 't', ...; 0 = the automatic / selected one)
    // batch: host hints, in_off[count] - in_off[0] and out_off[count] - out_off[0] (0 = unknown: the
    // K2j route and its workspace then read the offsets back, which waits for the stream)
    uint64_t in_bytes, out_bytes;
    // K2j, one stream (count == 1) continuing a Reader's stream (ez_reader_read's read-ahead, c_on):
    // the input is what the Reader has buffered, so it may end inside a token (the chain stops before
    // it); c_bsl: the window's log2 at the input's start (-1: none yet); c_hist: bytes of the window's
    // history right before out + out_off[0] (the last min(r.pos, len(r.block)) decoded bytes);
    // c_pos0: r.pos there (a MetaReset then hands the stream over unless c_pos0 and the output before
    // it are 0).  end_state then gets {window bytes, output bytes, input consumed by whole tokens, and
    // for a literal starting there whose body runs past the input its header length and length}
    int c_on;
    int32_t c_bsl;
    uint64_t c_hist;
    int64_t c_pos0;
    // batch, the size query (K2z, ez_decompressed_size_batch): the exact decoder reads every stream to
    // EOF with an unbounded capacity and stores nothing; out and out_off are not touched (may be null)
    int dry;
    // K2z's wave and lane kernels behind the parts route (ez_decompress_parts.hip), optional: they size
    // the whole batch where the device word size_gate is 0 (the parts route found the in_bytes hint too
    // small), else only the streams s without parts (size_base[s] == size_base[s + 1])
    const uint32_t *size_gate;
    const uint32_t *size_base;
    // batch, the Break index (K2b, ez_stream_breaks_batch), optional, the exact decoder run dry: the
    // count mode, brk_n[s] = the ErrBreaks of stream s before its first error; the fill mode (brk_out
    // set), Break k of stream s goes to brk_out[brk_base[s] + k], only the streams that own Breaks
    // (brk_base[s] != brk_base[s + 1]) are read, and nothing is done where the device word
    // brk_gate[0] is 0.  Null: the decoder does what it does without them (breaks above is the
    // Reader handles' one-stream counter, which these leave alone)
    uint64_t *brk_n;
    const uint64_t *brk_base;
    uint64_t *brk_out;
    const uint64_t *brk_gate;
};

// a fast path hands stream s over: appended to the slow list (one lane per stream calls this)
__device__ __forceinline__ void slow_append(const DecompressArgs &A, uint64_t s) {
    const uint32_t at = atomicAdd(&A.slow[0], 1u);
    A.slow[1 + at] = (uint32_t)s;
}

// words of workspace the two-level batch decoder needs
uint64_t decompress_workspace_words(uint64_t count);

hipError_t launch_compress(const CompressArgs &a, hipStream_t s);
// K1s: fresh streams, parse kernel + token-writer kernel (routed by ez_compress_split.hip to the
// families in ez_k1_*.hip); scratch = match records (+ the family's workspace), split_scratch_words
// u32 words
bool split_applies(const CompressArgs &a);  // K1s can take the batch
uint64_t split_scratch_words(const CompressArgs &a);
void select_split_table(bool t32);  // force the u32 exchange table (tests, A/B)
hipError_t launch_compress_split(const CompressArgs &a, uint32_t *scratch, hipStream_t s);
// the K1 kernel a batch launch takes: 's' K1s (parse + token writer), 'w' general wave per stream
char compress_variant(const CompressArgs &a);
void select_compress_variant(int v);  // 0 = automatic, else a variant letter (tests, A/B)
// the route of the last batch compress or Writer-handle call (ez_compress_route_last): every launcher
// stores the name of what it launched, a string literal; a launcher that calls another one (K1x, a
// handle call of several K1L Writes) stores its own last.  DESIGN §4 lists the names
void set_compress_route(const char *route);
const char *last_compress_route();
// K1L: the lean parse for long fresh streams (ez_k1_long.hip); resumes K1x's streams (spec_mode 2)
bool long_applies(const CompressArgs &a);
uint64_t long_scratch_bytes(const CompressArgs &a);
hipError_t launch_long(const CompressArgs &a, uint8_t *recs, hipStream_t s);
// K1L on a Writer handle's single Write (the handle's ring as history, its table in and out)
bool long_ring_applies(const CompressArgs &a);
// Writes up to this many bytes K1L stages in LDS (the input read once): the handle path then lets the
// kernels read the Write from, and write the output to, pinned host memory (no copies)
constexpr uint64_t kHandleLdsWrite = 49152;
uint64_t long_ring_scratch_bytes(const CompressArgs &a);
hipError_t launch_long_ring(const CompressArgs &a, uint8_t *recs, hipStream_t s);
// K1L on one Write of each of many handles in one launch (ez_writer_write_many): what block b needs
// of handle b's CompressArgs, in device memory; its in_off[2] out_off[2] out_size status words are
// the b-th six of the launch's meta words
struct RingDesc {
    uint8_t *ring;
    uint32_t *ht;
    int64_t bs, hs, start;
    int32_t header, append_magic;
};
uint64_t long_rings_scratch_bytes(uint64_t count, uint64_t longest);
hipError_t launch_long_rings(uint8_t *D, uint64_t *meta, const RingDesc *desc, uint64_t count, int64_t max_hs, uint64_t longest,
                             uint8_t *recs, hipStream_t s);
bool compress_forced_general();  // ez_select_compress_kernel('w') (tests, A/B)
bool compress_forced_long();     // ez_select_compress_kernel('l'): K1L alone, without K1c (tests, A/B)
// K1c (chunk-parallel K1L, ez_k1_chunk.hip): counting of its verdicts (ez_compress_k1c_stats)
bool chunk_applies(const CompressArgs &a);
void k1c_stats(int enable, uint64_t *out);
// K1x: the data-parallel first pass for long fresh single-Write streams (ez_compress_spec.hip)
bool spec_applies(const CompressArgs &a, bool any_len = false);  // any_len: also below 64 KiB (forced)
uint64_t spec_scratch_bytes(const CompressArgs &a);
hipError_t launch_compress_spec(const CompressArgs &a, uint8_t *scratch, hipStream_t s);
// the general kernel for one launch (ez_compress.hip); K1x calls it in its resume modes
hipError_t launch_general(const CompressArgs &a, hipStream_t s);
// u32 words of global hash-table scratch a batch launch needs (hs too big for LDS)
uint64_t compress_scratch_words(const CompressArgs &a);
hipError_t launch_decompress(const DecompressArgs &a, hipStream_t s);
void select_decompress_variant(int v);
int last_decompress_variant();  // the first K2 kernel of the last batch decode
// K2r: one lane per stream with a 512-byte LDS ring of recent output (ez_decompress_ring.hip)
hipError_t launch_decompress_ring(const DecompressArgs &a, hipStream_t s);
hipError_t launch_decompress_wave(const DecompressArgs &a, hipStream_t s);  // K2w, long streams
hipError_t launch_defer_copy(const DecompressArgs &a, hipStream_t s);       // kd_copy: K2t's (and K2w's) deferred literals
// K2j (ez_decompress_jump.hip): batches of at most 1,024 streams, chip-wide token starts, token
// records and pointer jumping over the copied bytes; streams it cannot take go to slow
bool jump_applies(const DecompressArgs &a);
uint64_t jump_workspace_bytes(uint64_t count, uint64_t in_total, uint64_t out_total);
// (hipErrorOutOfMemory: its workspace could not be had, nothing was launched)
hipError_t launch_decompress_jump(const DecompressArgs &a, hipStream_t s);
class DevCache;
DevCache &jump_cache();  // K2j's workspaces per (device, HIP stream)
// in_off[count] - in_off[0], out_off[count] - out_off[0]: the caller's hints, else read back (waits)
hipError_t batch_extents(const DecompressArgs &a, hipStream_t s, uint64_t *in_bytes, uint64_t *out_bytes);
hipError_t launch_decompress_tok(const DecompressArgs &a, hipStream_t s);   // K2t, token-parallel wave per stream
// K2z, the decoded-size query: the fast kernel (ez_decompress_size.hip; a.slow set, streams it cannot
// take go there), K2g's stage over that list (launch_size_segs) and then the exact decoder run dry over
// the stage's list, or that one alone (a.slow == nullptr); max_len:
// the caller's hint, the longest input stream (0 = unknown), which picks the fast kernel's chunk
hipError_t launch_decompress_size(const DecompressArgs &a, uint64_t max_len, hipStream_t s);
int size_chunk(uint64_t max_len);  // the wave kernel's chunk bytes for a hint
int size_route(uint64_t max_len, uint64_t count);  // 1: the lane-per-stream kernel; else the wave kernel's chunk
int last_size_chunk();             // the route of the last query (0: the exact decoder alone; -1: none yet)
hipError_t launch_size_fast(const DecompressArgs &a, int route, hipStream_t s);
// K2z's parts route (ez_decompress_parts.hip): every stream's chain cut over many waves, chunk 256 or
// 1,024; needs a.in_bytes.  probe: streams that start with tokens over half of them get no parts.
// *gate, *base: DecompressArgs.size_gate and size_base for the wave route launched behind it; lease: the scratch, held until that launch.  (hipErrorOutOfMemory: the scratch
// could not be had, nothing was launched)
int size_parts_route(uint64_t max_len, uint64_t count, uint64_t in_bytes);  // its chunk for a batch; 0: the wave route
// The part layout of this route and of K2g's (kp_layout, the steps of ez_k2_layout.h), chunk 256 or 1,024:
// zeroes the scratch's header hdr, then the gate, the batch's parts and base[0 .. count]; listed (may be
// null): count flags, cleared; cap: the records the scratch holds (parts_cap); probe: K2z's
hipError_t launch_parts_layout(int chunk, const uint8_t *in, const uint64_t *in_off, uint64_t count, uint64_t in_bytes, uint32_t *hdr, uint32_t *base,
                               uint32_t *listed, uint64_t cap, int probe, hipStream_t s);
class CacheLease;
hipError_t launch_size_parts(const DecompressArgs &a, int chunk, bool probe, hipStream_t s, CacheLease &lease, const uint32_t **gate,
                             const uint32_t **base);
uint64_t size_parts_workspace_bytes(uint64_t count, uint64_t in_bytes);  // its scratch where the caller owns it (a.jws / a.jws_cap)
DevCache &size_cache();            // its scratch per (device, HIP stream) otherwise
void select_size_route(int v);     // 0 = automatic, 'p' parts at any length, 'v' the wave route (tests, A/B)
int selected_size_route();
void size_parts_none();            // the last query did not take the parts route
hipError_t size_parts_last(uint64_t counts[3]);  // parts launched, taken as recorded, walked again
// K2g, the segment query (ez_decompress_segs.hip): where each stream can be cut at a MetaReset after
// output.  Stream s owns the segments seg_idx[s] .. seg_idx[s+1]-1; segment g is in[seg_in[g] ..
// seg_in[g+1]) decoded into out[seg_out[g] .. seg_out[g+1]) (out_off[s] plus the output before the cut,
// clamped to out_off[s+1]); seg_total = {segments written, segments found}: more found than seg_cap
// gives one segment per stream
struct SegsArgs {
    const uint8_t *in;
    const uint64_t *in_off;   // count+1
    const uint64_t *out_off;  // count+1
    uint64_t count;
    int64_t block_size_limit;
    uint64_t *seg_idx;        // count+1
    uint64_t *seg_in;         // seg_cap+1
    uint64_t *seg_out;        // seg_cap+1
    uint64_t seg_cap;         // >= count
    uint64_t *seg_total;      // 2
    uint32_t *hdr;            // the workspace's header and the cuts the count pass keeps (set by the launcher)
    uint64_t *keep;
    // the parts route (ez_decompress_segs_parts.hip), optional: in_bytes, the caller's hint of in_off[count]
    // - in_off[0] (0 = unknown: the wave route); pws / pws_cap, its scratch where the caller owns it
    // (segs_parts_workspace_bytes), else leased per (device, HIP stream).  parts_gate, parts_base (set by
    // the launcher): k2g_walk walks the whole batch where the device word parts_gate is 0 (the hint was
    // too small), else only the streams s without parts (parts_base[s] == parts_base[s + 1])
    uint64_t in_bytes;
    void *pws;
    uint64_t pws_cap;
    const uint32_t *parts_gate;
    const uint32_t *parts_base;
};
uint64_t segments_workspace_bytes(uint64_t count);
// max_len: the caller's hint, the longest input stream (0 = unknown), which picks the chunk (size_chunk)
hipError_t launch_segments(const SegsArgs &a, uint64_t max_len, void *workspace, hipStream_t s);
// K2g's parts route: every stream's chain cut over many waves, chunk 256 or 1,024; needs a.in_bytes.
// launch_segs_parts: layout, first and order passes (seg_idx[s] for the streams with parts, the parts'
// entry states); sets a's parts_gate / parts_base, and pws / pws_cap for launch_segs_parts_fill, which
// goes behind k2g_scan and k2g_heads.  lease: the scratch, held until the last launch.
// (hipErrorOutOfMemory: the scratch could not be had, nothing was launched)
int segs_parts_route(uint64_t max_len, uint64_t count, uint64_t in_bytes);  // its chunk for a batch; 0: the wave route
hipError_t launch_segs_parts(SegsArgs &a, int chunk, hipStream_t s, CacheLease &lease);
hipError_t launch_segs_parts_fill(const SegsArgs &a, int chunk, hipStream_t s);
uint64_t segs_parts_workspace_bytes(uint64_t count, uint64_t in_bytes);
// the size query's stage (launch_size_segs): the listed streams that have parts, by the first and order
// passes; *gate, *base: for k2g_size behind it
hipError_t launch_size_segs_parts(const DecompressArgs &a, int chunk, hipStream_t s, CacheLease &lease, const uint32_t **gate,
                                  const uint32_t **base);
DevCache &segs_parts_cache();
void select_segments_route(int v);  // 0 = automatic, 'p' parts at any length, 'v' the wave route (tests, A/B)
int selected_segments_route();
void segs_parts_none();             // the last query did not take the parts route
hipError_t segs_parts_last(uint64_t counts[4]);  // parts in the first pass, taken as recorded, walked again, filled
// per stream its first segment whose status is not EZ_OK, else its last: out_size[s] = seg_out[g] -
// out_off[s] + seg_size[g], status[s] (may be null) = seg_status[g]; slow, handed (optional): *handed =
// slow[0], the segments the fast decoders handed over
hipError_t launch_segments_merge(const uint64_t *out_off, uint64_t *out_size, int32_t *status, uint64_t count, const uint64_t *seg_idx,
                                 const uint64_t *seg_out, const uint64_t *seg_size, const int32_t *seg_status, const uint32_t *slow,
                                 uint64_t *handed, hipStream_t s);
// the query into scratch kept per (device, HIP stream), one read-back (which waits for the stream),
// launch_decompress over the segments, the merge; uses a's in, in_off, out, out_off, out_size, status,
// count and block_size_limit.  (hipErrorOutOfMemory: the scratch could not be had)
hipError_t launch_decompress_segmented(const DecompressArgs &a, hipStream_t s);
DevCache &segs_cache();
// K2g's stage of the size query (k2g_size, ez_decompress_segs.hip), behind K2z's kernels and before the
// exact decoder: the streams of a.slow's list that K2g's walk can size (concatenated streams) get their
// size and EZ_OK, the others go to a second list in the slow area's spare words.  size_segs_counters:
// the stage's words there, which the launcher zeroes first: {entries taken from the first list, streams
// sized, the second list: its length (the streams handed on), then its entries}
uint32_t *size_segs_counters(uint32_t *slow, uint64_t count);
// parts: the parts route's stage may take the listed streams that have parts (given a.in_bytes)
hipError_t launch_size_segs(const DecompressArgs &a, uint64_t max_len, hipStream_t s, bool parts);
hipError_t segments_last(uint64_t counts[3]);  // of the last segmented decode: segments, handed over, query retries
// K2b, the Break index (ez_decompress_brk.hip): stream s owns brk_pos[brk_idx[s] .. brk_idx[s+1]), the
// output positions of its Breaks; brk_total = {positions written, Breaks found}: more found than
// brk_cap writes none
struct BrkArgs {
    const uint8_t *in;
    const uint64_t *in_off;   // count+1
    uint64_t *out_size;       // count
    int32_t *status;          // count or nullptr
    uint64_t count;
    int64_t block_size_limit;
    uint64_t *brk_idx;        // count+1
    uint64_t *brk_pos;        // brk_cap (may be null with brk_cap == 0)
    uint64_t brk_cap;
    uint64_t *brk_total;      // 2
    uint32_t *list;           // the workspace's hand-over list, [0] = its length, and the per-stream
    uint32_t *handed;         // "handed over" words (set by the launcher)
    // the parts route (ez_decompress_brk_parts.hip), optional: in_bytes, the caller's hint of in_off[count]
    // - in_off[0] (0 = unknown: the wave route).  parts_gate, parts_base (set by the launcher): k2b_walk
    // walks the whole batch where the device word parts_gate is 0 (the hint was too small), else only
    // the streams s without parts (parts_base[s] == parts_base[s + 1])
    uint64_t in_bytes;
    const uint32_t *parts_gate;
    const uint32_t *parts_base;
};
uint64_t breaks_workspace_bytes(uint64_t count);
// K2b's parts route: a long stream's chain cut over many waves, chunk 256 or 1,024; needs a.in_bytes and
// the workspace (a.list, a.handed).  launch_breaks_parts: layout, first and order passes (out_size,
// status, brk_idx[s] = the Breaks, handed[s] or the list for the streams with parts; the parts' entry
// states); sets a's parts_gate / parts_base for k2b_walk behind it, and *pws for launch_breaks_parts_fill,
// which goes behind k2b_scan.  lease: the scratch, held until the last launch.
// (hipErrorOutOfMemory: the scratch could not be had, nothing was launched)
int breaks_parts_route(uint64_t max_len, uint64_t count, uint64_t in_bytes);  // its chunk for a batch; 0: the wave route
hipError_t launch_breaks_parts(BrkArgs &a, int chunk, hipStream_t s, CacheLease &lease, void **pws, uint64_t *pws_cap);
hipError_t launch_breaks_parts_fill(const BrkArgs &a, int chunk, void *pws, uint64_t pws_cap, hipStream_t s);
DevCache &breaks_parts_cache();
void select_breaks_route(int v);  // 0 = automatic, 'p' parts at any length, 'v' the wave route (tests, A/B)
int selected_breaks_route();
void breaks_parts_none();         // the last query did not take the parts route
hipError_t breaks_parts_last(uint64_t counts[4]);  // parts in the first pass, taken as recorded, walked again, filled
// max_len: the caller's hint, the longest input stream (0 = unknown), which picks the chunk (size_chunk);
// workspace null: the exact decoder alone
hipError_t launch_breaks(const BrkArgs &a, uint64_t max_len, void *workspace, hipStream_t s);
// the exact decoder run dry (a.dry) over a.slow's list, or over the whole batch without one
hipError_t launch_exact_dry(const DecompressArgs &a, hipStream_t s);
bool lds_exchange_in_lane_order();  // the LDS property K1s-T32 relies on (checked once, ez_k1_probe.hip)
bool lds_mskor_in_lane_order();     // the LDS property k1_lean's one-atomic visit relies on (checked once)
hipError_t launch_pack(const uint8_t *slots, const uint64_t *slot_off, const uint64_t *sizes, uint64_t count,
                       uint8_t *packed, uint64_t *packed_off, void *workspace, hipStream_t s);
size_t pack_workspace(uint64_t count);

}  // namespace ez
