/*
 * eazy.h — C-ABI of the MI355X-native eazy codec (libeazy_amd.so).
 *
 * This is the drop-in boundary a cgo shim binds (see INTEGRATION.md for the
 * Go side).  Plain pointers and sizes only.  Every entry point names the
 * reference (tlog-dev/eazy, Go) interface it replaces.
 *
 * Compute runs on AMD Instinct MI355X (gfx950) HIP kernels; there is no CPU
 * fallback: without a usable GPU every compute entry point returns
 * EZ_EDEVICE.  Only the scalar token codec (ez_encode_* / ez_decode_*) and
 * ez_compress_bound are host functions; they are the reference's exported
 * Encoder/Decoder value types, not the hot path.
 */
#ifndef EAZY_AMD_H
#define EAZY_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EZ_ABI_VERSION 2

/* ---- status codes: one per reference error value (reader.go:57-76) ---- */
enum {
    EZ_OK = 0,
    EZ_EOF = 1,            /* io.EOF */
    EZ_ESHORTBUF = 2,      /* ErrShortBuffer = io.ErrShortBuffer (reader.go:62) */
    EZ_EUNEXPECTEDEOF = 3, /* io.ErrUnexpectedEOF (reader.go:135-136) */
    EZ_EOVERFLOW = 4,      /* ErrOverflow (reader.go:61) */
    EZ_EBADMAGIC = 5,      /* ErrBadMagic (reader.go:58) */
    EZ_ENOMAGIC = 6,       /* ErrNoMagic (reader.go:60) */
    EZ_EBLOCKLIMIT = 7,    /* ErrBlockSizeOverLimit (reader.go:59) */
    EZ_EUNSUPMETA = 8,     /* ErrUnsupportedMeta (reader.go:63, 319) */
    EZ_EUNSUPVER = 9,      /* ErrUnsupportedVersion (reader.go:64, 303) */
    EZ_EBREAK = 10,        /* ErrBreak (reader.go:75) */
    EZ_EMISSEDMETA = 11,   /* errors.New("missed meta") (reader.go:155) */
    EZ_EINVAL = 12,        /* a reference panic: bad sizes (writer.go:162-168),
                              too big length/offset (:308-310, 562, 596), bad meta (:600-602) */
    EZ_ESINK = 13,         /* reserved for host shims: underlying io.Writer failed */
    EZ_ENOSPC = 14,        /* caller output buffer too small (C-ABI only) */
    EZ_EDEVICE = 15,       /* no usable MI355X / HIP runtime error */
    EZ_ESTUCK = 16         /* internal: a kernel's progress guard tripped */
};

/* ---- wire-format constants (writer.go:49-122) ---- */
#define EZ_LITERAL 0x00
#define EZ_COPY 0x80
#define EZ_META 0x80
#define EZ_LEN1 124
#define EZ_LEN2 125
#define EZ_LEN4 126
#define EZ_LEN_ALT 127
#define EZ_OFF1 252
#define EZ_OFF2 253
#define EZ_OFF4 254
#define EZ_OFF_LONG 255
#define EZ_META_MAGIC 0x00
#define EZ_META_VER 0x08
#define EZ_META_RESET 0x10
#define EZ_META_BREAK 0x18
#define EZ_META_LEN_WIDE 6
#define EZ_META_LEN0 7
#define EZ_VERSION 0

const char *ez_strerror(int code);

/* ---- which reference panic an EZ_EINVAL stands for, so a shim re-panics with Go's value ----
 * ez_encode_tag: always EZ_PANIC_LENGTH (writer.go:562); ez_encode_offset: EZ_PANIC_OFFSET
 * (:596); ez_encode_meta: EZ_PANIC_META when meta & ~0xf8 (:600-602, Go panics with the meta
 * int), else EZ_PANIC_OFFSET (its wide length goes through Offset); a Writer handle:
 * ez_writer_last_panic; NewWriter / ResetSize: ez_writer_size_panic. */
enum {
    EZ_PANIC_NONE = 0,
    EZ_PANIC_BLOCK = 1,  /* "block size must be a power of two (32 < bs < 1<<31)" writer.go:163 */
    EZ_PANIC_HTABLE = 2, /* "hash table size must be a power of two (hs >= 4)"    writer.go:167 */
    EZ_PANIC_LENGTH = 3, /* "too big length"                                       writer.go:562 */
    EZ_PANIC_OFFSET = 4, /* "too big offset"                                       writer.go:309, 596 */
    EZ_PANIC_META = 5    /* panic(meta)                                            writer.go:601 */
};
const char *ez_panic_message(int panic);
int ez_writer_size_panic(int64_t block, int64_t htable); /* Writer.init writer.go:161-169; 0 = valid */
int ez_abi_version(void);
/* Number of visible HIP devices (0 when none). */
int ez_device_count(void);

/* ---- low-level token codec: Encoder (writer.go:537-621), Decoder (reader.go:346-514) ----
 * Encoders append at b[*len] (cap = total capacity of b); EZ_EINVAL where Go panics.
 * Decoders mirror Go's (…, i, err) results: *i is `st` on any error. */
int ez_encode_tag(uint8_t *b, size_t cap, size_t *len, int tag, int64_t l);       /* Encoder.Tag    writer.go:537 */
int ez_encode_offset(uint8_t *b, size_t cap, size_t *len, int64_t off, int64_t l); /* Encoder.Offset writer.go:565 */
int ez_encode_meta(uint8_t *b, size_t cap, size_t *len, int64_t meta, int64_t l);  /* Encoder.Meta   writer.go:599 */
int ez_decode_tag(const uint8_t *b, size_t n, size_t st, int *tag, int64_t *l, size_t *i);       /* Decoder.Tag    reader.go:346 */
int ez_decode_offset(const uint8_t *b, size_t n, size_t st, int64_t l, int64_t *off, size_t *i); /* Decoder.Offset reader.go:394 */
int ez_decode_meta(const uint8_t *b, size_t n, size_t st, int64_t *meta, int64_t *l, size_t *i); /* Decoder.Meta   reader.go:474 */

/* Upper bound of the bytes one Write of n bytes can append (header included).
 * Derived (not in the reference); proved in tests/test_bound.py. */
size_t ez_compress_bound(size_t n);

/* ---- streaming Writer handle: the state of writer.go Writer (:17-46) ----
 * The ring (block), hash table and stream position live in HBM on `device`.
 * The io.Writer sink, the output buffer b, FlushThreshold and `written` stay
 * in the host shim (writer.go:379-401); the handle tracks isreset()
 * (writer.go:403) as "nothing emitted since the last reset". */
typedef struct ez_writer ez_writer;
int ez_writer_new(int64_t block, int64_t htable, int device, ez_writer **out); /* NewWriter writer.go:133 */
void ez_writer_free(ez_writer *w);
int ez_writer_set_append_magic(ez_writer *w, int on); /* Writer.AppendMagic writer.go:25 */
int ez_writer_set_version(ez_writer *w, int ver);     /* Writer.e.Ver writer.go:21 */
/* Writer.Write(p) writer.go:206-337: compresses p on the GPU and returns in
 * out[0..*out_n) exactly the bytes Go appends to w.b for this call (header
 * included on a pristine stream).  cap >= ez_compress_bound(n). */
int ez_writer_write(ez_writer *w, const uint8_t *p, size_t n, uint8_t *out, size_t cap, size_t *out_n);
/* k Writes on the handle in one device call, the same as k ez_writer_write calls in
 * turn: p holds the Writes back to back, Write j ending at p[ends[j]] (ends
 * non-decreasing); out receives their bytes back to back, Write j's ending at
 * out[out_ends[j]].  cap >= the sum of ez_compress_bound(len of Write j).  The
 * mirrors replay FlushThreshold per Write from out_ends, so a caller batching small
 * Writes sees the reference's sink calls (writer.go:379-401).  Errors as
 * ez_writer_write (the stream restarts). */
int ez_writer_write_batch(ez_writer *w, const uint8_t *p, const uint64_t *ends, size_t k, uint8_t *out, size_t cap,
                          uint64_t *out_ends);
/* One Write on each of `count` distinct handles in one device call: the same bytes, handle states and
 * errors as ez_writer_write(w[j], ...) for j = 0 .. count-1.  p holds the Writes back to back, handle j's
 * ending at p[ends[j]]; out receives their bytes back to back, handle j's ending at out[out_ends[j]].
 * cap >= the sum of ez_compress_bound(len of Write j).  status (may be NULL) gets EZ_* per handle.
 * Returns EZ_OK when every Write succeeded, else the first failing handle's code.  A handle whose Write
 * fails restarts its stream as after ez_writer_write and contributes no bytes (out_ends[j] ==
 * out_ends[j-1]); the others keep their results.  Refused before anything reaches a device, every
 * handle as it was: EZ_EINVAL for a NULL w, ends or out_ends, a NULL handle, decreasing ends, a handle
 * named twice or handles on different devices; EZ_ENOSPC for cap below the sum of the bounds.  count ==
 * 0 returns EZ_OK.  The handles need not share a block size, table size, AppendMagic or state.  Writes
 * of 16 .. 49,152 bytes on handles with version 0, a table of at most 4,096 entries and a block of at
 * most 2^26 that end at or before stream position 2^32 share one launch, a block of threads per
 * handle; every other Write runs as ez_writer_write does, after that launch, inside the call.  Thread
 * safety is the handles': no handle of the call may be in use by another thread. */
int ez_writer_write_many(ez_writer *const *w, size_t count, const uint8_t *p, const uint64_t *ends,
                         uint8_t *out, size_t cap, uint64_t *out_ends, int32_t *status);
/* Introspection (tests, measurement): of the last ez_writer_write_many call of this process, how many
 * Writes ran in the shared launch (counts[0]) and how many on their handle's own path (counts[1]). */
int ez_writer_write_many_last(uint64_t counts[2]);
int ez_writer_header(ez_writer *w, uint8_t *out, size_t cap, size_t *out_n); /* WriteHeader writer.go:342 */
int ez_writer_break(ez_writer *w, uint8_t *out, size_t cap, size_t *out_n);  /* WriteBreak  writer.go:358 */
int ez_writer_reset(ez_writer *w);                                          /* Reset       writer.go:149 (reset :187) */
int ez_writer_reset_size(ez_writer *w, int64_t block, int64_t htable);     /* ResetSize   writer.go:155 */
int ez_writer_is_reset(const ez_writer *w);                                 /* isreset     writer.go:403 */
int ez_writer_last_panic(const ez_writer *w); /* EZ_PANIC_* behind the handle's last EZ_EINVAL */
/* Testing hook (no reference counterpart): set w.pos, ring and table unchanged, so a test can
 * run Writes across stream position 2^32, where the table's uint32 values (writer.go:216-217)
 * stop matching; the C oracle has the same hook. */
int ez_writer_set_position(ez_writer *w, int64_t pos);

/* ---- streaming Reader handle: the decoder state of reader.go Reader (:17-40) ----
 * Window, position and current token live on the device.  The host shim owns
 * r.b / r.i / r.boff and the refill from io.Reader (more(), reader.go:516-543). */
typedef struct ez_reader ez_reader;
int ez_reader_new(int device, ez_reader **out); /* NewReader / NewReaderBytes reader.go:79, 89 */
void ez_reader_free(ez_reader *r);
/* Reader.BlockSizeLimit, RequireMagic, SkipUnsupportedMeta (reader.go:27-30) */
int ez_reader_configure(ez_reader *r, int64_t block_size_limit, int require_magic, int skip_unsupported_meta);
int ez_reader_reset(ez_reader *r); /* the decoder part of ResetBytes reader.go:102-113 */
/* The inner loop of Reader.Read (reader.go:119-133) without the refill:
 * decodes from b[i..b_len) (boff = absolute offset of b[0]) into p until p is
 * full (EZ_OK), the input runs short (EZ_ESHORTBUF: caller refills and calls
 * again), or another error.  *n = bytes produced, *i_out = new r.i,
 * *detail = meta id / version for EZ_EUNSUPMETA / EZ_EUNSUPVER. */
int ez_reader_read(ez_reader *r, const uint8_t *b, size_t b_len, size_t i, int64_t boff, uint8_t *p,
                   size_t p_len, size_t *n, size_t *i_out, int64_t *detail);
int ez_reader_pending(const ez_reader *r); /* r.state != 0 (reader.go:135) */
/* The b of this handle's Reads is the whole stream (NewReaderBytes / ResetBytes with no
 * io.Reader behind it; no reference counterpart): the first Read of a fresh stream then decodes
 * all of it at once on the device and the Reads are served from that output -- the same bytes,
 * ErrBreak / errors / EOF at the same Reads (streams with a Break meta, an error, RequireMagic
 * or SkipUnsupportedMeta keep the Read-by-Read decode). 0 (default): b may grow (NewReader). */
int ez_reader_set_whole(ez_reader *r, int whole);
/* 1 when this stream's Reads are being served from the whole-stream decode (tests, measurement). */
int ez_reader_whole_decoded(const ez_reader *r);
/* Introspection (tests, measurement) of the last whole-stream attempt (the first Read of a set_whole
 * handle): the capacity in bytes of the slot it decoded into (the stream's decoded size from the size
 * query, rounded up to 16; 0 if it decoded nothing: the query gave an error or a size over 1 GiB, and
 * the Reads are decoded one by one), and the number of decode launches it made (0 or 1). */
uint64_t ez_reader_whole_slot(const ez_reader *r);
int ez_reader_whole_launches(const ez_reader *r);
/* NewReader(io.Reader) handles (set_whole 0) read ahead: a Read with nothing decoded ahead and at
 * least 8 KiB of buffered input b[i..b_len) decodes every whole token of it at once on the device
 * (K2j continuing the stream from the handle's state, a literal the buffer ends inside of decoded as
 * far as it goes), and the Reads are served from that output -- the same bytes, ErrBreak and errors at
 * the same Reads as Read by Read, and ErrShortBuffer (the shim's refill, more()) with *i_out where
 * Read by Read would ask for more input.  A buffer the device path hands over (an error, a MetaReset
 * after output, ...) is decoded Read by Read until more input arrives.  The number of read-aheads
 * this handle has made (tests, measurement): */
int64_t ez_reader_ahead_count(const ez_reader *r);

/* ---- device-resident batches of independent streams (the GPU hot path) ----
 * One stream = a fresh NewWriter(block, htable) receiving one Write; its
 * bytes equal Go's `NewWriter(&buf, block, htable).Write(p)` output.
 * All pointers below are DEVICE pointers on the current HIP device; calls
 * are asynchronous on `hip_stream` (a hipStream_t, NULL = default stream). */
typedef struct {
    const uint8_t *in;       /* concatenated inputs */
    const uint64_t *in_off;  /* count+1 offsets into in */
    uint8_t *out;            /* output slots */
    const uint64_t *out_off; /* count+1 offsets: slot s = out[out_off[s] .. out_off[s+1]) */
    uint64_t *out_size;      /* count: bytes written into each slot */
    int32_t *status;         /* count: EZ_* per stream (may be NULL) */
    uint64_t count;
    /* host hint: max input length of a stream (decompress: max slot; 0 = unknown).  Compress: the hint
     * sizes the route's scratch and picks the route, nothing else -- a larger hint gives the same
     * bytes; a stream of exactly max_len bytes is accepted; a longer one (a multi-Write stream: its
     * Writes together) gets status EZ_EINVAL and out_size 0, nothing is written into its slot and
     * the other streams are untouched; 0 = unknown takes the general kernel. */
    uint64_t max_len;
    /* decompress, host hints (ABI 2): in_off[count] - in_off[0] and out_off[count] - out_off[0],
     * both 0 = unknown.  With them the decoder route and its workspace need no read-back of the
     * offsets, so the call never waits for the stream; compress ignores them.  The hints count only
     * as a pair: one alone is taken as unknown (the offsets are read back).  A wrong hint costs
     * speed, never memory safety: the decoder checks the pair against the offsets on the device
     * before it indexes anything sized from them, and a batch larger than its hints is decoded by
     * the exact decoder (same bytes, sizes and statuses); larger hints only enlarge the workspace. */
    uint64_t in_bytes;
    uint64_t out_bytes;
} ez_batch;

#define EZ_F_NO_MAGIC 0x1 /* compress: AppendMagic = false */

/* K1: compress every stream of b into its slot (slot >= ez_compress_bound(n)).  Held by
 * tests/test_gpu_k1_edges.py and tests/test_gpu_k1_hints.py; at offsets past 2^31 and 2^32 and on
 * batches larger than 4 GiB by tests/test_gpu_high_offsets.py. */
int ez_compress_batch(int64_t block, int64_t htable, int flags, const ez_batch *b, void *hip_stream);
/* K1 for streams that each receive several Writes (Writer.Write writer.go:206
 * called k times on one NewWriter, FlushThreshold 0: the slot holds what the
 * sink receives over the k calls).  Stream s receives the Writes
 * k = write_idx[s] .. write_idx[s+1]-1 (device arrays, write_idx[count+1]);
 * Write k is in[prev .. write_end[k]) with prev = in_off[s] for the first.
 * max_writes: the most Writes of one stream (host hint; it reserves the records of the
 * Writes' ends).  A stream with more Writes is refused: status EZ_ESTUCK, out_size 0,
 * nothing written into its slot, the other streams untouched.  Slots need
 * ez_compress_bound(n) + 5 bytes per Write.  Streams of any length: K1s takes
 * batches with 2 x length <= block, the general kernel the others. */
int ez_compress_batch_writes(int64_t block, int64_t htable, int flags, const ez_batch *b, const uint64_t *write_idx,
                             const uint64_t *write_end, uint64_t max_writes, void *hip_stream);
/* K3: exclusive scan of sizes -> packed_off[count+1], then gather the slots
 * densely into packed.  workspace >= ez_pack_workspace(count) device bytes.
 * Stream s is slots[slot_off[s] .. slot_off[s] + sizes[s]); it lands at
 * packed[packed_off[s] .. packed_off[s+1]).  slots, packed and every
 * slot_off[s] may have any byte alignment (slot_off, sizes, packed_off and
 * workspace are uint64 arrays, 8-aligned); sizes[s] may be 0; slots may lie in
 * any order, with gaps, adjacent or overlapping (they are only read).
 * packed_off[0] = 0 whatever slot_off[0] is, and only packed[0 .. packed_off[count])
 * and packed_off[0 .. count] are written.  The source is read in whole aligned
 * dwords that hold a byte of a stream, so up to 3 bytes either side of it (never
 * outside a page the stream lies in; the bytes are read, not used).
 * count == 0 writes packed_off[0] only.  The workspace's contents on entry are ignored: it need
 * not be cleared, and may hold what any earlier call left.  Held by tests/test_gpu_k3_pack.py. */
size_t ez_pack_workspace(uint64_t count);
int ez_pack_batch(const uint8_t *slots, const uint64_t *slot_off, const uint64_t *sizes, uint64_t count,
                  uint8_t *packed, uint64_t *packed_off, void *workspace, void *hip_stream);
/* K2: decode every compressed stream b->in[in_off[s]..in_off[s+1]) completely
 * (NewReaderBytes + read to EOF; ErrBreak markers are skipped) into its slot.
 * status[s] = EZ_OK on a clean end of stream, else the first error;
 * out_size[s] = bytes produced before it (out_size is required).
 * workspace >= ez_decompress_workspace(count) device bytes enables the
 * lane-per-stream fast decoder (streams it cannot take are handed to the
 * exact wave-per-stream decoder); NULL = exact decoder only.
 * Memory touched: in[0 .. in_off[count]) must be readable (the decoders' clamped loads may read
 * any byte of it, bytes before in_off[0] included; none is read at or past in_off[count], and no
 * result depends on a byte outside the streams), and in_off holds at least 16 bytes.  Nothing
 * outside the slots is written.  A stream with status EZ_OK leaves its slot's bytes from
 * out_size[s] on untouched; a stream with an error may leave part of its slot overwritten (a fast
 * decoder's output before the hand-over), never a byte outside it.  A fast decoder takes only
 * slots of at least 16 bytes and batches of at least 16 input bytes; the others go to the exact
 * decoder.  Held by tests/test_gpu_k2r.py, test_gpu_k2t.py and test_gpu_k2j.py; at offsets past
 * 2^31 and 2^32, at slots of 2^30 bytes and more and on batches larger than 4 GiB by
 * tests/test_gpu_high_offsets.py.
 * The workspace's contents on entry are ignored: it need not be cleared, it may hold what any
 * earlier call left there (this call's, the size query's, another batch's), and nothing is written
 * past ez_decompress_workspace(count) bytes.  out_size[s] and status[s] are written for every
 * stream of the batch, empty and refused ones included.  Scratch the library keeps between calls
 * carries nothing from one call to the next (see ez_release_cached).  The same holds for
 * ez_decompressed_size_batch and ez_decompress_batch_segmented. */
size_t ez_decompress_workspace(uint64_t count);
int ez_decompress_batch(int64_t block_size_limit, const ez_batch *b, void *workspace, void *hip_stream);
/* K2z: what ez_decompress_batch would report for every stream given a slot that is large enough,
 * without decoding: out_size[s] = the bytes NewReaderBytes(in_s) read to EOF produces (Break metas
 * skipped; for a stream that ends in an error, the bytes produced before it), status[s] = EZ_OK or
 * that first error.  Uses b->in, in_off, out_size (required), status (may be NULL), count and
 * max_len (host hint: the longest INPUT stream in bytes, 0 = unknown; it picks the chunk size and
 * nothing else: any value gives the same results) and in_bytes (host hint: in_off[count] -
 * in_off[0], 0 = unknown; it enables the parts route below and nothing else: any value gives the
 * same results).  b->out, out_off and out_bytes are ignored (out and out_off may be NULL).  workspace >= ez_decompress_workspace(count) enables the
 * fast kernel (streams it cannot take go to the exact decoder run dry); NULL = exact decoder only.
 * The fast kernel is a wave per stream, or, for 4,096 streams or more of at most 4 KiB (max_len), a
 * lane per stream; or the parts route: every stream's token chain cut on a fixed grid of parts of 64
 * chunks, a wave per part and then a wave per stream that follows the true chain through the parts'
 * records and walks again only the parts it enters elsewhere.  The parts route sizes its records from
 * in_bytes, so it runs only where the caller gives in_bytes (and the route is selected, see
 * ez_select_size_route); a kernel checks the real extent against the hint before anything indexes
 * those records, and an under-stated hint leaves the whole batch to the wave route (an over-stated one
 * only enlarges the scratch, which is kept per (device, HIP stream) and freed by ez_release_cached;
 * if it cannot be had the call takes the wave route).  Asynchronous on hip_stream; never waits for the stream.  Reads in[0 .. in_off[count]) as
 * ez_decompress_batch does; writes only out_size[0..count), status[0..count) and the workspace.
 * Sizes are 64-bit throughout: an output over 4 GiB is reported, not clamped.
 * Held by tests/test_gpu_k2z.py, tests/test_k2_size.py, tests/test_gpu_k2z_parts.py,
 * tests/test_k2_size_parts.py and (offsets past 2^31 and 2^32) tests/test_gpu_high_offsets.py. */
int ez_decompressed_size_batch(int64_t block_size_limit, const ez_batch *b, void *workspace, void *hip_stream);
/* Introspection (tests, tuning): the chunk bytes the fast kernel takes for a max_len hint (host function). */
int ez_decompressed_size_chunk(uint64_t max_len);
/* the chunk bytes the last call of this process ran with (0: exact decoder alone; -1: none yet;
 * 1: the lane-per-stream kernel, which batches of 4,096 streams or more take when max_len says they
 * are at most 4 KiB each: no chunks) */
int ez_decompressed_size_chunk_last(void);
/* Testing / A-B measurement: the fast route of later ez_decompressed_size_batch calls in this
 * process: 'p' the parts route at any stream length (it still needs b->in_bytes; chunk 1,024 where
 * the wave route takes 1,024, else 256), 'v' never the parts route, 0 = automatic.  EZ_EINVAL for
 * any other value.  Not thread-safe against concurrent calls. */
int ez_select_size_route(int kind);
/* Introspection (tests, measurement): of the last ez_decompressed_size_batch call of this process,
 * counts[0] = parts the parts route walked in its first pass, counts[1] = parts whose record the
 * true chain took as it stood, counts[2] = parts walked again from the true entry (parts a token
 * spans are in neither); all 0 where the parts route did not run or found in_bytes too small.  The
 * caller has synchronised that call's stream; the call reads the counters back from the device. */
int ez_decompressed_size_parts_last(uint64_t counts[3]);
/* Concatenated streams in the size query (a MetaReset after output, see K2g below): the fast kernels
 * hand such a stream over, and a stage behind them walks every handed-over stream as
 * ez_stream_segments_batch does, a wave per stream, keeping the total instead of the cuts.  A stream
 * whose walk ends at its input's end with every segment passing the fast decoders' checks gets
 * out_size[s] = the total and EZ_OK there; every other one goes on to the exact decoder run dry.  The
 * stage keeps three counters in the workspace, which this call reads back: counts[0] = streams the fast
 * kernels handed over, counts[1] = those the stage sized, counts[2] = those it handed on to the exact
 * decoder (counts[0] = counts[1] + counts[2]).  workspace and count are those of an
 * ez_decompressed_size_batch call with a workspace whose stream the caller has synchronised; count ==
 * 0 gives zeros.  EZ_EINVAL for a NULL workspace or counts.  A caller that decodes next takes
 * ez_decompress_batch_segmented where counts[1] != 0, so that the decode leaves the exact decoder too.
 * Held by tests/test_k2_segs_size.py and tests/test_gpu_size_segments.py. */
int ez_decompressed_size_segs_last(const void *workspace, uint64_t count, uint64_t counts[3]);

/* K2g: concatenated streams.  A stream may hold a MetaReset after output (reader.go:305-311, 327-344: a
 * Writer that was Reset, or streams joined back to back); ez_decompress_batch hands such a stream to
 * the exact decoder whole.  Reader.reset zeroes the block and sets r.pos = 0, so the stream is as many
 * independent streams as it has such Resets, plus one, and this query finds them: a *cut* is a
 * MetaReset on the stream's token chain with output before it in the stream (Resets before the first
 * output byte stay in segment 0; a Reset with no output since the previous cut is still a cut: empty
 * segments are allowed).  A cut is recorded only if the segment it closes would be taken by the fast
 * decoders (no form they hand over, a window set before its first token, its longest distance within
 * its window); at the first segment that is not, and for a stream of 2 GiB or more, the walk of that
 * stream stops: the cuts so far stand and the rest of the stream is its last segment, which the
 * decoders then see exactly as they see the whole stream today.
 * Stream s owns the segments seg_idx[s] .. seg_idx[s+1]-1 (seg_idx[count+1]); segment g is
 * in[seg_in[g] .. seg_in[g+1]) decoded into out[seg_out[g] .. seg_out[g+1]) (absolute offsets in the
 * style of in_off / out_off, seg_cap+1 entries each).  seg_in[seg_idx[s]] = in_off[s]; a cut's seg_in
 * is the position of the Reset's 0x80 tag byte (padding before it belongs to the segment before);
 * its seg_out is out_off[s] plus the output before the cut, clamped to out_off[s+1] (a stream whose
 * slot is too small ends in segments of short or zero capacity).  Both arrays end at in_off[count]
 * and out_off[count].  seg_total[0] = the segments written, seg_total[1] = the segments found: where
 * those exceed seg_cap the one-segment-per-stream layout is written instead (seg_idx[s] = s, the
 * offsets equal to in_off / out_off) and seg_total = {count, found}, so that a caller can retry with room.
 * Uses b->in, in_off, out_off, count, max_len (host hint: the longest INPUT stream in bytes, 0 =
 * unknown; it picks the chunk size and nothing else) and in_bytes (host hint: in_off[count] -
 * in_off[0] or more, 0 = unknown; it enables the parts route below and nothing else: any value gives
 * the same arrays).  workspace >= ez_segments_workspace(count) device bytes.
 * The walk is a wave per stream, or, for the few long streams that one wave each would bound, the
 * parts route: every stream's chain cut on K2z's fixed grid of parts of 64 chunks; a wave per part
 * writes a record that can be applied to any incoming state (cuts, window, longest distance since the
 * last cut, stop); a wave per stream follows the true chain through the records, walks again only the
 * parts it enters elsewhere or in which the stream stops, and leaves every part's entry state; a wave
 * per part that holds a Reset then writes that part's cuts in place.  The route sizes its scratch from
 * in_bytes, so it runs only where the caller gives in_bytes (and the route is selected, see
 * ez_select_segments_route); a kernel checks the real extent against the hint before anything indexes
 * the scratch, and an under-stated hint leaves the whole batch to the wave route (an over-stated one
 * only enlarges the scratch, which is kept per (device, HIP stream) and freed by ez_release_cached; if
 * it cannot be had the call takes the wave route).  EZ_EINVAL for a NULL array or workspace or seg_cap < count; count == 0 writes
 * seg_idx[0], seg_in[0], seg_out[0] and seg_total and returns EZ_OK.
 * Asynchronous on hip_stream; never waits for the stream.  Memory touched: reads in[0 .. in_off[count])
 * as ez_decompress_batch does, in_off and out_off; no output buffer is needed; writes only
 * seg_idx[0 .. count], seg_in and seg_out[0 .. seg_total[0]], seg_total[0 .. 1] and the workspace.
 * The workspace's contents on entry are ignored: it need not be cleared, and nothing is written past
 * ez_segments_workspace(count) bytes; the parts route's scratch is the library's own.
 * Held by tests/test_k2_segments.py, tests/test_gpu_segments.py, tests/test_k2_segs_parts.py,
 * tests/test_gpu_segments_parts.py and (offsets past 2^31 and 2^32) tests/test_gpu_high_offsets.py. */
size_t ez_segments_workspace(uint64_t count);
int ez_stream_segments_batch(int64_t block_size_limit, const ez_batch *b, uint64_t *seg_idx, uint64_t *seg_in, uint64_t *seg_out,
                             uint64_t seg_cap, uint64_t *seg_total, void *workspace, void *hip_stream);
/* Testing / A-B measurement: the route of later segment queries in this process (ez_stream_segments_batch
 * and the query inside ez_decompress_batch_segmented): 'p' the parts route at any stream length (it
 * still needs b->in_bytes; chunk 1,024 where the wave route takes 1,024, else 256), 'v' never the parts
 * route, 0 = automatic.  EZ_EINVAL for any other value.  Not thread-safe against concurrent calls.
 * Host function: touches no device memory. */
int ez_select_segments_route(int kind);
/* Introspection (tests, measurement): of the last ez_stream_segments_batch or
 * ez_decompressed_size_batch call of this process, whichever came later (the size query's stage over
 * the handed-over streams that have parts: it fills nothing, and a size query with a workspace that
 * does not take the route zeroes the counters), counts[0] = parts the parts route walked in its first pass, counts[1] = parts whose record the true
 * chain took as it stood, counts[2] = parts walked again from the true state (parts a token spans are
 * in neither), counts[3] = parts whose cuts the fill pass wrote; all 0 where the parts route did not run
 * or found in_bytes too small, and for the query inside ez_decompress_batch_segmented, whose scratch is
 * that call's.  The caller has synchronised that call's stream.  Memory touched: the call reads 64
 * bytes of the library's own scratch back from the device and writes counts[0 .. 3]; EZ_EINVAL for NULL. */
int ez_segments_parts_last(uint64_t counts[4]);
/* The results of a decode over segments, per stream: g = the stream's first segment whose
 * seg_status is not EZ_OK, else its last; out_size[s] = seg_out[g] - out_off[s] + seg_size[g],
 * status[s] (may be NULL) = seg_status[g].  Uses b->out_off, out_size, status and count.
 * Asynchronous on hip_stream.  Memory touched: reads out_off[0 .. count), seg_idx[0 .. count] and the
 * three segment arrays up to seg_idx[count]; writes only out_size[0 .. count) and status[0 .. count). */
int ez_segments_merge_batch(const ez_batch *b, const uint64_t *seg_idx, const uint64_t *seg_out, const uint64_t *seg_size,
                            const int32_t *seg_status, void *hip_stream);
/* ez_decompress_batch for batches whose streams may be concatenated: the same out, out_size and status,
 * with every segment on the fast decoders.  In order: ez_stream_segments_batch into scratch the
 * library keeps per (device, HIP stream) (freed by ez_release_cached); one read-back of seg_total and
 * the decode's hints, WHICH WAITS FOR THE STREAM; the query once more where the segments found exceeded
 * the room; ez_decompress_batch's decoders over the segments, with the library's own workspace (always
 * the fast decoders first); ez_segments_merge_batch.  A batch without any Reset after output costs the
 * query and then exactly ez_decompress_batch's decode.  Uses b->in, in_off, out, out_off, out_size
 * (required), status (may be NULL), count and in_bytes (the query's hint as for
 * ez_stream_segments_batch: in_off[count] - in_off[0] or more, 0 = unknown; an over-statement such as
 * the compressed buffer's length only enlarges the scratch, and any value gives the same results);
 * max_len and out_bytes are ignored (the call measures what the decode needs).  workspace is accepted
 * for symmetry and may be NULL.
 * Memory touched: as ez_decompress_batch; nothing outside the slots, out_size and status is written. */
int ez_decompress_batch_segmented(int64_t block_size_limit, const ez_batch *b, void *workspace, void *hip_stream);
/* Introspection (tests, measurement): of the last ez_decompress_batch_segmented call of this process,
 * counts[0] = segments decoded, counts[1] = how many of them the fast decoders handed to the exact
 * decoder, counts[2] = query retries.  The caller has synchronised that call's stream; the call reads
 * counts[1] back from the library's scratch (0 once ez_release_cached freed it). */
int ez_segments_last(uint64_t counts[3]);

/* K2b: the Break index.  Writer.WriteBreak (writer.go:352-366) writes a two-byte marker that separates
 * chunks of data in one stream; Reader.Read returns ErrBreak there and stays valid (reader.go:66-75,
 * :312-313).  The batch decoders above skip the markers; this query lists them, for every stream of a
 * batch, without decoding: a stream's Breaks are the ErrBreaks NewReaderBytes(in_s) read to EOF returns
 * before its first error, in order, and a Break's position is the number of bytes the Reader has
 * produced when the ErrBreak comes back: the offset into the slot ez_decompress_batch fills, relative
 * to the slot's start.  Positions do not decrease; two Breaks with no output between them give the
 * same position twice (an empty message); a Break before any output has position 0; a stream that
 * holds MetaResets after output counts its output across all of them, as the slot does; nothing after
 * the first error is listed.
 * Stream s owns brk_pos[brk_idx[s] .. brk_idx[s+1]) (brk_idx[count+1], the exclusive scan of the
 * streams' Break counts: always written in full, always the true counts).  brk_total[1] = the Breaks
 * found (= brk_idx[count]), brk_total[0] = the positions written: all of them, or, where the Breaks
 * found exceed brk_cap, none (no entry of brk_pos is written), so that a caller can retry with room.
 * brk_pos may be NULL when brk_cap is 0.  out_size[s] and status[s] are exactly what
 * ez_decompressed_size_batch reports.
 * Uses b->in, in_off, out_size (required), status (may be NULL), count and max_len (host hint: the
 * longest INPUT stream in bytes, 0 = unknown; it picks the chunk size as ez_decompressed_size_chunk
 * says and nothing else: any value gives the same arrays) and in_bytes (host hint: in_off[count] -
 * in_off[0] or more, 0 = unknown; it enables the parts route below and nothing else: any value gives
 * the same arrays); out, out_off and out_bytes are
 * ignored.  workspace >= ez_breaks_workspace(count) device bytes enables the fast walk (a wave per
 * stream over the true token chain, once to count and, for the streams that own Breaks, once more to
 * write; streams it cannot take go whole to the exact decoder run dry); NULL = the exact decoder alone,
 * with the same results.  The workspace's contents on entry are ignored and nothing is written past
 * its size.
 * The parts route, for the few long streams that one wave each would bound: every stream's chain cut
 * on K2z's fixed grid of parts of 64 chunks; a wave per part writes K2g's state-independent record and
 * the part's Breaks; a wave per stream follows the true chain through the records, walks again only
 * the parts it enters elsewhere or that are marked, leaves every part's entry state and the stream's
 * verdict (all or nothing: a stream it cannot take goes whole to the exact decoder); a wave per part
 * whose chain holds a Break then writes that part's positions in place.  The route sizes its scratch
 * from in_bytes, so it runs only where the caller gives in_bytes and a workspace (and the route is
 * selected, see ez_select_breaks_route); a kernel checks the real extent against the hint before
 * anything indexes the scratch, and an under-stated hint leaves the whole batch to the wave route (an
 * over-stated one only enlarges the scratch, which is the library's own, kept per (device, HIP
 * stream) and freed by ez_release_cached; if it cannot be had the call takes the wave route).
 * All pointers are device pointers.  Asynchronous on hip_stream; never waits for the stream.
 * Memory touched: reads in[0 .. in_off[count]) as ez_decompress_batch does; writes only
 * out_size[0..count), status[0..count), brk_idx[0..count], brk_pos[0..brk_total[0]), brk_total[0..1]
 * and the workspace.  EZ_EINVAL for a NULL b, out_size, brk_idx or brk_total, and for a NULL brk_pos
 * with brk_cap != 0; count == 0 writes brk_idx[0] = 0 and brk_total = {0, 0} and returns EZ_OK.
 * Held by tests/test_k2_breaks.py, tests/test_capi_breaks.py, tests/test_gpu_breaks.py,
 * tests/test_cpp_breaks.py, tests/test_k2_brk_parts.py, tests/test_gpu_breaks_parts.py and (offsets
 * past 2^31 and 2^32) tests/test_gpu_high_offsets.py. */
size_t ez_breaks_workspace(uint64_t count);
int ez_stream_breaks_batch(int64_t block_size_limit, const ez_batch *b, uint64_t *brk_idx, uint64_t *brk_pos, uint64_t brk_cap,
                           uint64_t *brk_total, void *workspace, void *hip_stream);
/* Testing / A-B measurement: the route of later ez_stream_breaks_batch calls in this process: 'p' the
 * parts route at any stream length (it still needs b->in_bytes and a workspace; chunk 1,024 where the
 * wave route takes 1,024, else 256), 'v' never the parts route, 0 = automatic (today: the wave route).
 * EZ_EINVAL for any other value.  Not thread-safe against concurrent calls.
 * Host function: touches no device memory. */
int ez_select_breaks_route(int kind);
/* Introspection (tests, measurement): of the last ez_stream_breaks_batch call of this process,
 * counts[0] = parts the parts route walked in its first pass, counts[1] = parts whose record the true
 * chain took as it stood, counts[2] = parts walked again from the true state (parts a token spans are
 * in neither), counts[3] = parts whose Break positions the fill pass wrote; all 0 where the parts route
 * did not run or found in_bytes too small.  The caller has synchronised that call's stream.  Memory
 * touched: the call reads 64 bytes of the library's own scratch back from the device and writes
 * counts[0 .. 3]; EZ_EINVAL for NULL. */
int ez_breaks_parts_last(uint64_t counts[4]);

/* ---- host-memory batches over several devices (SURVEY §8b device_or_all) ----
 * Streams share no state (writer.go:40-45, reader.go:17-40), so a batch splits into contiguous
 * whole-stream shards, balanced by bytes, one per entry of `devices` (ndev entries; NULL or 0 =
 * every visible device; an entry may repeat: two shards on one device, each on its own HIP
 * stream); each shard runs on its own host thread: upload, the batch kernels, download.  All
 * pointers are HOST pointers; the calls return when the output is in host memory.
 * Shard k begins with the first stream that starts at or after k / ndev of the batch's bytes
 * (eazy_amd/csrc/ez_multi_shards.h, held on the host by tests/test_multi_shards.py); a shard may be
 * empty, and each shard takes its own route from its own longest stream and byte counts.
 *
 * Compress: stream s = in[in_off[s] .. in_off[s+1]) as one Write to a fresh NewWriter(block,
 * htable); packed gets the streams' outputs back to back, packed_off[count+1] their offsets
 * (a host exclusive scan of the shards' packed sizes), status[count] (may be NULL) EZ_* per
 * stream.  packed_cap < packed_off[count] -> EZ_ENOSPC with packed_off filled, packed untouched
 * (sum of ez_compress_bound(n) always suffices).  EZ_EINVAL for invalid sizes, a NULL in_off or
 * packed_off, an in_off that decreases anywhere (all checked before any device use) or a device
 * entry that does not exist: nothing is written then, packed_off[0] neither.
 * Held by tests/test_gpu_multi_edges.py (the oracle at every shard edge) and tests/test_gpu_batch.py. */
int ez_compress_batch_multi(int64_t block, int64_t htable, int flags, const uint8_t *in, const uint64_t *in_off, uint64_t count,
                            const int *devices, int ndev, uint8_t *packed, uint64_t packed_cap, uint64_t *packed_off,
                            int32_t *status);
/* Decompress: stream s = in[in_off[s] .. in_off[s+1]) read to EOF as NewReaderBytes does (Break
 * metas skipped) into out[out_off[s] .. out_off[s+1]); out_size[count] bytes produced,
 * status[count] (may be NULL) EZ_OK or the first error, as ez_decompress_batch.  On this host
 * path the bytes of a slot past out_size[s] are unspecified (each shard's whole device range is
 * copied down, whatever its pooled buffer held).  EZ_EINVAL for a NULL in_off, out_off or out_size,
 * an in_off or out_off that decreases anywhere (all checked before any device use) or a device entry
 * that does not exist: nothing is written then.
 * Held by tests/test_gpu_multi_edges.py (the oracle at every shard edge), tests/test_gpu_batch.py and
 * tests/test_gpu_size_multi.py. */
int ez_decompress_batch_multi(int64_t block_size_limit, const uint8_t *in, const uint64_t *in_off, uint64_t count,
                              const int *devices, int ndev, uint8_t *out, const uint64_t *out_off, uint64_t *out_size,
                              int32_t *status);
/* Decoded sizes: what ez_decompress_batch_multi would report for every stream given slots that are
 * large enough, without decoding and without an output (ez_decompressed_size_batch on every shard,
 * with each shard's max_len and in_bytes hints): out_size[count] and status[count] (may be NULL).
 * A caller that does not know its decoded lengths lays its slots out from out_size (a host prefix
 * sum) and then calls ez_decompress_batch_multi.  EZ_EINVAL for NULL in_off or out_size or an in_off
 * that decreases anywhere (checked before any device use, nothing written); count == 0 returns EZ_OK.
 * Held by tests/test_gpu_multi_edges.py (the oracle at every shard edge) and tests/test_gpu_size_multi.py. */
int ez_decompressed_size_batch_multi(int64_t block_size_limit, const uint8_t *in, const uint64_t *in_off, uint64_t count,
                                     const int *devices, int ndev, uint64_t *out_size, int32_t *status);

/* Frees the device scratch kept between batch calls (no reference counterpart; a caching
 * allocator's empty_cache).  The set: per (device, HIP stream), the K1 / K1c / K1x scratch of
 * ez_compress_batch and _writes, the K2j workspaces of ez_decompress_batch, the parts routes' scratch
 * of ez_decompressed_size_batch, ez_stream_segments_batch and ez_stream_breaks_batch, ez_decompress_batch_segmented's scratch and ez_writer_write_many's
 * staging (device and pinned); per device, the Reader handles' shared K2j workspace; and the
 * multi-device calls' pooled shard buffers.  device < 0 = every device.  Scratch in use by a
 * concurrent call is kept.  Entries beyond 8 streams per device are also freed least recently used
 * first as new streams arrive.
 * Scratch kept between calls carries nothing from one call to the next: every call gives the results
 * it would give on freshly allocated scratch of any contents (held by tests/test_gpu_dirty_scratch.py
 * and tests/test_gpu_call_order.py). */
int ez_release_cached(int device);
/* Testing / introspection: sets every idle buffer of the set ez_release_cached frees (the same
 * set: the per-(device, HIP stream) scratch of K1 / K1c / K1x, K2j, the three parts routes,
 * ez_decompress_batch_segmented and ez_writer_write_many, device and pinned; the Reader handles'
 * shared K2j workspace; the multi-device calls' pooled shard buffers) to `byte` (0..255), or touches
 * nothing and only counts with byte = -1; *bytes (may be NULL) gets the device and pinned bytes
 * covered.  device < 0 = every device.  Scratch a concurrent call holds is skipped.  Waits for the
 * device before it fills and before it returns.  EZ_EINVAL for any other byte or a device that does
 * not exist. */
int ez_fill_cached(int device, int byte, uint64_t *bytes);
/* Introspection (tests, measurement): the shards of the last ez_*_batch_multi call in this process
 * (returns their number; up to cap entries filled, any pointer may be NULL): each shard's device and
 * its device interval (upload to download) in ms from the earliest shard start on that device.
 * Empty shards are not counted; with cap below the number, the number is still returned.
 * Held by tests/test_gpu_multi_edges.py. */
int ez_multi_last_shards(int *dev, double *t0_ms, double *t1_ms, int cap);

/* Introspection (no reference counterpart): the K1 kernel a batch of `count`
 * fresh streams of <= max_len bytes would run on the current device, as a
 * character: 's' K1s (parse + token writer; fresh streams with 2n <= block and
 * at most 4096 table entries), 'x' K1x (data-parallel rounds over the emitting
 * positions, then the general kernel; other fresh single-Write batches of streams
 * up to 2 GiB, at least one of 64 KiB or more, at most 4096 table entries),
 * 'w' general wave per stream (everything else);
 * EZ_EDEVICE (negated) without a device. */
int ez_compress_kernel(int64_t block, int64_t htable, uint64_t max_len, uint64_t count);
/* Testing / A-B measurement (no reference counterpart): force the K1 kernel of
 * later batch calls in this process ('s' K1s, 'S' K1s with the u32
 * exchange table, 'w' general alone, 'x' K1x at any stream length, 'l' K1L alone (the lean
 * parse for long fresh streams, which otherwise continues K1x's dense streams); 0 = automatic choice).  A forced kernel that cannot take a batch falls
 * back to the automatic choice.  Not thread-safe against concurrent calls. */
int ez_select_compress_kernel(int kind);
/* Testing / A-B measurement: the first K2 kernel of later batch decodes with a
 * workspace ('r' lane-per-stream with an LDS ring of recent output, 't'
 * token-parallel wave per stream, 'w' wave per stream with a scalar token walk; 0 = automatic:
 * 't' when a slot is 64 KiB or more, else 'r'; the largest
 * slot is max_len when the caller gives it, else measured on the device, which waits for the
 * stream).  Streams the chosen kernel cannot take go on to the exact decoder. */
int ez_select_decompress_kernel(int kind);
/* Introspection: the first K2 kernel the last ez_decompress_batch call of this process ran
 * ('r', 't', 'w'; 'e' the exact decoder alone; 0 none yet). */
int ez_decompress_kernel_last(void);
/* Introspection (tests, measurement): the route the last ez_compress_batch / _writes call of this
 * process took, as a short NUL-terminated string; returns its length (0: none yet).  "s:lean g16 fw40"
 * (k1_lean: lanes per stream, the judgement's forward bytes), "s:parse t32", "s:parse t16 mw"
 * (k1_parse: table width, multi-Write), "l" (K1L), "l:k1c" (K1c, K1L behind it), "x" (K1x),
 * "w:pl" / "w:win" / "w:view" (the general kernel: stream staged in LDS, 32 KiB LDS window, global
 * view), "+gtab" appended when its hash tables are in global scratch.  A Writer handle's call stores
 * its route too: "hl:lds" / "hl:global" (K1L on the handle's ring, the Write staged in LDS / read from
 * global memory), "hl:batch zero-copy" / "hl:batch staged" (several such Writes in one call), "hw:pl" /
 * "hw:view" / "hw:multi" (the general kernel on the ring: one Write staged in LDS, one in the global
 * view, several Writes in one launch), "+gtab" appended when the table has more than 4096 entries.
 * ez_writer_write_many stores "hm:lds" (every Write shared its launch), "hm:lds+own" (some ran on
 * their handle's own path) or "hm:own" (none shared the launch). */
int ez_compress_route_last(char *buf, int cap);
/* Testing: K1c (the chunk-parallel parse of long fresh streams, which proves each stream's parse
 * is Go's or gives it to K1L) counts its verdicts while counting is on: counts (6 words, may be
 * NULL) gets {streams proven, chunk error or re-visit, no common copy end, a judgement changed,
 * record slot, path segments} so far; enable 1 clears them and turns counting on (each K1c batch
 * then waits for its verdicts), 0 turns it off. */
int ez_compress_k1c_stats(int enable, uint64_t *counts);

#ifdef __cplusplus
}
#endif
#endif /* EAZY_AMD_H */
