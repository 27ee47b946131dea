package eazy

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#include <stdint.h>
#include "eazy.h"
#include <hip/hip_runtime_api.h>
#cgo LDFLAGS: -L/opt/rocm/lib -lamdhip64
*/
import "C"

import (
	"errors"
	"unsafe"
)

// compressBatch: one stream per buffer (one Write each), through ez_compress_batch_multi: the
// batch is split into contiguous whole-stream shards over every visible device (Devices, when set),
// one host thread and HIP stream per device, and the packed result comes back in host memory.
func compressBatch(bufs [][]byte, block, htable int) ([][]byte, error) {
	sizePanic(block, htable) // Writer.init writer.go:161-169, as NewWriter would
	count := len(bufs)
	if count == 0 {
		return nil, nil
	}
	inOff := make([]uint64, count+1)
	capacity := uint64(16)
	for k, b := range bufs {
		inOff[k+1] = inOff[k] + uint64(len(b))
		capacity += uint64(C.ez_compress_bound(C.size_t(len(b))))
	}
	host := make([]byte, 0, inOff[count]+1)
	for _, b := range bufs {
		host = append(host, b...)
	}
	host = append(host, 0) // (a valid pointer for an all-empty batch)
	packed := make([]byte, capacity)
	packedOff := make([]uint64, count+1)
	status := make([]int32, count)
	var devs *C.int
	ndev := 0
	if len(Devices) > 0 {
		cd := make([]C.int, len(Devices))
		for k, d := range Devices {
			cd[k] = C.int(d)
		}
		devs, ndev = &cd[0], len(cd)
	}
	st := C.ez_compress_batch_multi(C.int64_t(block), C.int64_t(htable), 0, (*C.uint8_t)(unsafe.Pointer(&host[0])),
		(*C.uint64_t)(unsafe.Pointer(&inOff[0])), C.uint64_t(count), devs, C.int(ndev), (*C.uint8_t)(unsafe.Pointer(&packed[0])),
		C.uint64_t(capacity), (*C.uint64_t)(unsafe.Pointer(&packedOff[0])), (*C.int32_t)(unsafe.Pointer(&status[0])))
	if st != C.EZ_OK {
		return nil, toErr(st, 0)
	}
	res := make([][]byte, count)
	for k := range bufs {
		if status[k] != 0 {
			return nil, errors.Join(ErrDevice, toErr(C.int(status[k]), 0))
		}
		res[k] = packed[packedOff[k]:packedOff[k+1]:packedOff[k+1]]
	}
	return res, nil
}

// compressStreams stages the streams into device memory, runs K1 (stream k =
// NewWriter(block, htable) receiving the Writes streams[k] in order,
// FlushThreshold 0) and copies every slot back.  One HIP stream per call.
func compressStreams(streams [][][]byte, block, htable int) ([][]byte, error) {
	sizePanic(block, htable) // Writer.init writer.go:161-169, as NewWriter would
	count := len(streams)
	if count == 0 {
		return nil, nil
	}
	inOff := make([]uint64, count+1)
	outOff := make([]uint64, count+1)
	writeIdx := make([]uint64, count+1)
	var writeEnd []uint64
	maxLen, maxWrites, multi := 0, 1, false
	for k, ws := range streams {
		n := 0
		for _, w := range ws {
			n += len(w)
			writeEnd = append(writeEnd, inOff[k]+uint64(n))
		}
		if len(ws) != 1 {
			multi = true
		}
		if len(ws) > maxWrites {
			maxWrites = len(ws)
		}
		inOff[k+1] = inOff[k] + uint64(n)
		writeIdx[k+1] = uint64(len(writeEnd))
		outOff[k+1] = outOff[k] + uint64(C.ez_compress_bound(C.size_t(n))) + 5*uint64(len(ws))
		if n > maxLen {
			maxLen = n
		}
	}
	host := make([]byte, 0, inOff[count])
	for _, ws := range streams {
		for _, w := range ws {
			host = append(host, w...)
		}
	}
	var dIn, dOut, dInOff, dOutOff, dSize, dStatus, dWIdx, dWEnd unsafe.Pointer
	alloc := func(p *unsafe.Pointer, n uint64) error {
		if C.hipMalloc(p, C.size_t(n+16)) != C.hipSuccess {
			return ErrDevice
		}
		return nil
	}
	defer func() {
		for _, p := range []unsafe.Pointer{dIn, dOut, dInOff, dOutOff, dSize, dStatus, dWIdx, dWEnd} {
			if p != nil {
				C.hipFree(p)
			}
		}
	}()
	// every HIP call's result is checked: a failed copy must never hand back stale bytes as success
	// (the errors surface as the reference's do, writer.go:387-401)
	hip := func(r C.hipError_t) error {
		if r != C.hipSuccess {
			return ErrDevice
		}
		return nil
	}
	for _, a := range []struct {
		p *unsafe.Pointer
		n uint64
	}{{&dIn, inOff[count]}, {&dOut, outOff[count]}, {&dInOff, 8 * uint64(count+1)}, {&dOutOff, 8 * uint64(count+1)},
		{&dSize, 8 * uint64(count)}, {&dStatus, 4 * uint64(count)}, {&dWIdx, 8 * uint64(count+1)},
		{&dWEnd, 8 * uint64(len(writeEnd))}} {
		if err := alloc(a.p, a.n); err != nil {
			return nil, err
		}
	}
	if len(host) > 0 {
		if err := hip(C.hipMemcpy(dIn, unsafe.Pointer(&host[0]), C.size_t(len(host)), C.hipMemcpyHostToDevice)); err != nil {
			return nil, err
		}
	}
	if err := hip(C.hipMemcpy(dInOff, unsafe.Pointer(&inOff[0]), C.size_t(8*(count+1)), C.hipMemcpyHostToDevice)); err != nil {
		return nil, err
	}
	if err := hip(C.hipMemcpy(dOutOff, unsafe.Pointer(&outOff[0]), C.size_t(8*(count+1)), C.hipMemcpyHostToDevice)); err != nil {
		return nil, err
	}
	b := C.ez_batch{
		in: (*C.uint8_t)(dIn), in_off: (*C.uint64_t)(dInOff), out: (*C.uint8_t)(dOut), out_off: (*C.uint64_t)(dOutOff),
		out_size: (*C.uint64_t)(dSize), status: (*C.int32_t)(dStatus), count: C.uint64_t(count), max_len: C.uint64_t(maxLen),
	}
	var st C.int
	if multi {
		if err := hip(C.hipMemcpy(dWIdx, unsafe.Pointer(&writeIdx[0]), C.size_t(8*(count+1)), C.hipMemcpyHostToDevice)); err != nil {
			return nil, err
		}
		if len(writeEnd) > 0 {
			if err := hip(C.hipMemcpy(dWEnd, unsafe.Pointer(&writeEnd[0]), C.size_t(8*len(writeEnd)), C.hipMemcpyHostToDevice)); err != nil {
				return nil, err
			}
		}
		st = C.ez_compress_batch_writes(C.int64_t(block), C.int64_t(htable), 0, &b, (*C.uint64_t)(dWIdx),
			(*C.uint64_t)(dWEnd), C.uint64_t(maxWrites), nil)
	} else {
		st = C.ez_compress_batch(C.int64_t(block), C.int64_t(htable), 0, &b, nil)
	}
	if st != C.EZ_OK {
		return nil, toErr(st, 0)
	}
	out := make([]byte, outOff[count])
	size := make([]uint64, count)
	status := make([]int32, count)
	// (hipMemcpy to host waits for the batch's kernels on the null stream, and reports their faults)
	if err := hip(C.hipMemcpy(unsafe.Pointer(&out[0]), dOut, C.size_t(len(out)), C.hipMemcpyDeviceToHost)); err != nil {
		return nil, err
	}
	if err := hip(C.hipMemcpy(unsafe.Pointer(&size[0]), dSize, C.size_t(8*count), C.hipMemcpyDeviceToHost)); err != nil {
		return nil, err
	}
	if err := hip(C.hipMemcpy(unsafe.Pointer(&status[0]), dStatus, C.size_t(4*count), C.hipMemcpyDeviceToHost)); err != nil {
		return nil, err
	}
	res := make([][]byte, count)
	for k := range streams {
		if status[k] != 0 {
			return nil, errors.Join(ErrDevice, toErr(C.int(status[k]), 0))
		}
		res[k] = out[outOff[k] : outOff[k]+size[k]]
	}
	return res, nil
}

// decompressedSizes: every stream's decoded length without decoding (ez_decompressed_size_batch).
// The streams are staged into device memory, the query runs on the null stream with the fast kernel's
// workspace, and the lengths and statuses come back; a stream's own error is returned as the
// reference's Reader would report it, with the bytes it produced before it in sizes[k].
func decompressedSizes(streams [][]byte, blockSizeLimit int) ([]uint64, []error, error) {
	count := len(streams)
	if count == 0 {
		return nil, nil, nil
	}
	inOff := make([]uint64, count+1)
	maxLen := 0
	for k, s := range streams {
		inOff[k+1] = inOff[k] + uint64(len(s))
		if len(s) > maxLen {
			maxLen = len(s)
		}
	}
	host := make([]byte, 0, inOff[count])
	for _, s := range streams {
		host = append(host, s...)
	}
	var dIn, dInOff, dSize, dStatus, dWork unsafe.Pointer
	defer func() {
		for _, p := range []unsafe.Pointer{dIn, dInOff, dSize, dStatus, dWork} {
			if p != nil {
				C.hipFree(p)
			}
		}
	}()
	// every HIP call's result is checked: a failed copy must never hand back stale sizes as success
	hip := func(r C.hipError_t) error {
		if r != C.hipSuccess {
			return ErrDevice
		}
		return nil
	}
	for _, a := range []struct {
		p *unsafe.Pointer
		n uint64
	}{{&dIn, inOff[count]}, {&dInOff, 8 * uint64(count+1)}, {&dSize, 8 * uint64(count)}, {&dStatus, 4 * uint64(count)},
		{&dWork, uint64(C.ez_decompress_workspace(C.uint64_t(count)))}} {
		if err := hip(C.hipMalloc(a.p, C.size_t(a.n+16))); err != nil {
			return nil, nil, err
		}
	}
	if len(host) > 0 {
		if err := hip(C.hipMemcpy(dIn, unsafe.Pointer(&host[0]), C.size_t(len(host)), C.hipMemcpyHostToDevice)); err != nil {
			return nil, nil, err
		}
	}
	if err := hip(C.hipMemcpy(dInOff, unsafe.Pointer(&inOff[0]), C.size_t(8*(count+1)), C.hipMemcpyHostToDevice)); err != nil {
		return nil, nil, err
	}
	b := C.ez_batch{
		in: (*C.uint8_t)(dIn), in_off: (*C.uint64_t)(dInOff), out_size: (*C.uint64_t)(dSize), status: (*C.int32_t)(dStatus),
		count: C.uint64_t(count), max_len: C.uint64_t(maxLen),
	}
	if st := C.ez_decompressed_size_batch(C.int64_t(blockSizeLimit), &b, dWork, nil); st != C.EZ_OK {
		return nil, nil, toErr(st, 0)
	}
	sizes := make([]uint64, count)
	status := make([]int32, count)
	// (hipMemcpy to host waits for the query's kernels on the null stream, and reports their faults)
	if err := hip(C.hipMemcpy(unsafe.Pointer(&sizes[0]), dSize, C.size_t(8*count), C.hipMemcpyDeviceToHost)); err != nil {
		return nil, nil, err
	}
	if err := hip(C.hipMemcpy(unsafe.Pointer(&status[0]), dStatus, C.size_t(4*count), C.hipMemcpyDeviceToHost)); err != nil {
		return nil, nil, err
	}
	errs := make([]error, count)
	for k := range streams {
		if status[k] != 0 {
			errs[k] = toErr(C.int(status[k]), 0)
		}
	}
	return sizes, errs, nil
}

// decompressedSizesMulti: every stream's decoded length without decoding, from host memory over
// several devices (ez_decompressed_size_batch_multi; devices nil: every visible device).  The call
// stages, queries and reads back per shard and returns when the lengths are in host memory; its
// return code covers every HIP call it made, and is checked before any length is used.  A stream's
// own error is returned as the reference's Reader would report it, with the bytes it produced
// before it in sizes[k].
func decompressedSizesMulti(streams [][]byte, blockSizeLimit int, devices []int) ([]uint64, []error, error) {
	count := len(streams)
	if count == 0 {
		return nil, nil, nil
	}
	inOff := make([]uint64, count+1)
	for k, s := range streams {
		inOff[k+1] = inOff[k] + uint64(len(s))
	}
	host := make([]byte, 0, inOff[count]+1)
	for _, s := range streams {
		host = append(host, s...)
	}
	host = append(host, 0) // (never read: &host[0] must exist for a batch of empty streams)
	var devs *C.int
	cdev := make([]C.int, len(devices))
	for k, d := range devices {
		cdev[k] = C.int(d)
	}
	if len(cdev) > 0 {
		devs = &cdev[0]
	}
	sizes := make([]uint64, count)
	status := make([]int32, count)
	st := C.ez_decompressed_size_batch_multi(C.int64_t(blockSizeLimit), (*C.uint8_t)(unsafe.Pointer(&host[0])),
		(*C.uint64_t)(unsafe.Pointer(&inOff[0])), C.uint64_t(count), devs, C.int(len(cdev)),
		(*C.uint64_t)(unsafe.Pointer(&sizes[0])), (*C.int32_t)(unsafe.Pointer(&status[0])))
	if st != C.EZ_OK {
		return nil, nil, toErr(st, 0)
	}
	errs := make([]error, count)
	for k := range streams {
		if status[k] != 0 {
			errs[k] = toErr(C.int(status[k]), 0)
		}
	}
	return sizes, errs, nil
}

// DecompressBatchSegmented decodes independent streams that may each be several streams joined back
// to back, or the output of a Writer that was Reset (a MetaReset after output), on the GPU
// (ez_decompress_batch_segmented): the segment query cuts every stream at such Resets and the batch
// decoders take one segment each.  caps[k] is the room for stream k's output; the result for
// streams[k] is what NewReaderBytes(streams[k]) read to EOF produces, with the Reader's error in
// errs[k] (EZ_ENOSPC's error where caps[k] is too small).  The streams are staged into device
// memory, the call runs on the null stream, and the outputs, lengths and statuses come back; every
// HIP call's result is checked before anything is used.
func DecompressBatchSegmented(streams [][]byte, caps []uint64, blockSizeLimit int) ([][]byte, []error, error) {
	count := len(streams)
	if count == 0 {
		return nil, nil, nil
	}
	if len(caps) != count {
		return nil, nil, toErr(C.EZ_EINVAL, 0)
	}
	inOff := make([]uint64, count+1)
	outOff := make([]uint64, count+1)
	for k, s := range streams {
		inOff[k+1] = inOff[k] + uint64(len(s))
		outOff[k+1] = outOff[k] + caps[k]
	}
	host := make([]byte, 0, inOff[count])
	for _, s := range streams {
		host = append(host, s...)
	}
	var dIn, dOut, dInOff, dOutOff, dSize, dStatus unsafe.Pointer
	defer func() {
		for _, p := range []unsafe.Pointer{dIn, dOut, dInOff, dOutOff, dSize, dStatus} {
			if p != nil {
				C.hipFree(p)
			}
		}
	}()
	// every HIP call's result is checked: a failed copy must never hand back stale bytes as success
	hip := func(r C.hipError_t) error {
		if r != C.hipSuccess {
			return ErrDevice
		}
		return nil
	}
	for _, a := range []struct {
		p *unsafe.Pointer
		n uint64
	}{{&dIn, inOff[count]}, {&dOut, outOff[count]}, {&dInOff, 8 * uint64(count+1)}, {&dOutOff, 8 * uint64(count+1)},
		{&dSize, 8 * uint64(count)}, {&dStatus, 4 * uint64(count)}} {
		if err := hip(C.hipMalloc(a.p, C.size_t(a.n+16))); err != nil {
			return nil, nil, err
		}
	}
	if len(host) > 0 {
		if err := hip(C.hipMemcpy(dIn, unsafe.Pointer(&host[0]), C.size_t(len(host)), C.hipMemcpyHostToDevice)); err != nil {
			return nil, nil, err
		}
	}
	if err := hip(C.hipMemcpy(dInOff, unsafe.Pointer(&inOff[0]), C.size_t(8*(count+1)), C.hipMemcpyHostToDevice)); err != nil {
		return nil, nil, err
	}
	if err := hip(C.hipMemcpy(dOutOff, unsafe.Pointer(&outOff[0]), C.size_t(8*(count+1)), C.hipMemcpyHostToDevice)); err != nil {
		return nil, nil, err
	}
	b := C.ez_batch{
		in: (*C.uint8_t)(dIn), in_off: (*C.uint64_t)(dInOff), out: (*C.uint8_t)(dOut), out_off: (*C.uint64_t)(dOutOff),
		out_size: (*C.uint64_t)(dSize), status: (*C.int32_t)(dStatus), count: C.uint64_t(count),
		in_bytes: C.uint64_t(inOff[count]), // (the query's parts route needs the extent)
	}
	if st := C.ez_decompress_batch_segmented(C.int64_t(blockSizeLimit), &b, nil, nil); st != C.EZ_OK {
		return nil, nil, toErr(st, 0)
	}
	out := make([]byte, outOff[count]+1)
	size := make([]uint64, count)
	status := make([]int32, count)
	// (hipMemcpy to host waits for the call's kernels on the null stream, and reports their faults)
	if outOff[count] > 0 {
		if err := hip(C.hipMemcpy(unsafe.Pointer(&out[0]), dOut, C.size_t(outOff[count]), C.hipMemcpyDeviceToHost)); err != nil {
			return nil, nil, err
		}
	}
	if err := hip(C.hipMemcpy(unsafe.Pointer(&size[0]), dSize, C.size_t(8*count), C.hipMemcpyDeviceToHost)); err != nil {
		return nil, nil, err
	}
	if err := hip(C.hipMemcpy(unsafe.Pointer(&status[0]), dStatus, C.size_t(4*count), C.hipMemcpyDeviceToHost)); err != nil {
		return nil, nil, err
	}
	res := make([][]byte, count)
	errs := make([]error, count)
	for k := range streams {
		if size[k] > caps[k] {
			return nil, nil, ErrDevice // (never: a size is at most its slot)
		}
		res[k] = out[outOff[k] : outOff[k]+size[k] : outOff[k]+size[k]]
		if status[k] != 0 {
			errs[k] = toErr(C.int(status[k]), 0)
		}
	}
	return res, errs, nil
}

// StreamBreaksBatch lists the Breaks of independent streams on the GPU without decoding them
// (ez_stream_breaks_batch, K2b): breaks[k] holds, for every ErrBreak that NewReaderBytes(streams[k])
// read to EOF returns before its first error, the bytes the Reader has produced by then, in order:
// offsets into the stream's decoded output (what DecompressBatchSegmented returns for it), so that
// out[breaks[k][j-1]:breaks[k][j]] is message j.  sizes[k] is the decoded length and errs[k] the
// Reader's error, as the size query reports them.  The streams are staged into device memory and the
// calls run on the null stream; where the Breaks found exceed the room of the first call, the query
// runs once more with room.  Every HIP call's result is checked before anything is used.
func StreamBreaksBatch(streams [][]byte, blockSizeLimit int) (breaks [][]uint64, sizes []uint64, errs []error, err error) {
	count := len(streams)
	if count == 0 {
		return nil, nil, nil, nil
	}
	inOff := make([]uint64, count+1)
	maxLen := 0
	for k, s := range streams {
		inOff[k+1] = inOff[k] + uint64(len(s))
		if len(s) > maxLen {
			maxLen = len(s)
		}
	}
	host := make([]byte, 0, inOff[count])
	for _, s := range streams {
		host = append(host, s...)
	}
	var dIn, dInOff, dSize, dStatus, dIdx, dPos, dTotal, dWork unsafe.Pointer
	defer func() {
		for _, p := range []unsafe.Pointer{dIn, dInOff, dSize, dStatus, dIdx, dPos, dTotal, dWork} {
			if p != nil {
				C.hipFree(p)
			}
		}
	}()
	// every HIP call's result is checked: a failed copy must never hand back stale words as success
	hip := func(r C.hipError_t) error {
		if r != C.hipSuccess {
			return ErrDevice
		}
		return nil
	}
	for _, a := range []struct {
		p *unsafe.Pointer
		n uint64
	}{{&dIn, inOff[count]}, {&dInOff, 8 * uint64(count+1)}, {&dSize, 8 * uint64(count)}, {&dStatus, 4 * uint64(count)},
		{&dIdx, 8 * uint64(count+1)}, {&dTotal, 16}, {&dWork, uint64(C.ez_breaks_workspace(C.uint64_t(count)))}} {
		if err := hip(C.hipMalloc(a.p, C.size_t(a.n+16))); err != nil {
			return nil, nil, nil, err
		}
	}
	if len(host) > 0 {
		if err := hip(C.hipMemcpy(dIn, unsafe.Pointer(&host[0]), C.size_t(len(host)), C.hipMemcpyHostToDevice)); err != nil {
			return nil, nil, nil, err
		}
	}
	if err := hip(C.hipMemcpy(dInOff, unsafe.Pointer(&inOff[0]), C.size_t(8*(count+1)), C.hipMemcpyHostToDevice)); err != nil {
		return nil, nil, nil, err
	}
	b := C.ez_batch{
		in: (*C.uint8_t)(dIn), in_off: (*C.uint64_t)(dInOff), out_size: (*C.uint64_t)(dSize), status: (*C.int32_t)(dStatus),
		count: C.uint64_t(count), max_len: C.uint64_t(maxLen),
		in_bytes: C.uint64_t(inOff[count]), // (the query's parts route needs the extent)
	}
	room := uint64(4*count + 64)
	var total [2]uint64
	for try := 0; ; try++ {
		if err := hip(C.hipMalloc(&dPos, C.size_t(8*room+16))); err != nil {
			return nil, nil, nil, err
		}
		if st := C.ez_stream_breaks_batch(C.int64_t(blockSizeLimit), &b, (*C.uint64_t)(dIdx), (*C.uint64_t)(dPos), C.uint64_t(room),
			(*C.uint64_t)(dTotal), dWork, nil); st != C.EZ_OK {
			return nil, nil, nil, toErr(st, 0)
		}
		// (hipMemcpy to host waits for the query's kernels on the null stream, and reports their faults)
		if err := hip(C.hipMemcpy(unsafe.Pointer(&total[0]), dTotal, 16, C.hipMemcpyDeviceToHost)); err != nil {
			return nil, nil, nil, err
		}
		if total[1] <= room {
			break
		}
		if try != 0 {
			return nil, nil, nil, ErrDevice // (never: the second call has the room the first one asked for)
		}
		if err := hip(C.hipFree(dPos)); err != nil {
			return nil, nil, nil, err
		}
		dPos = nil
		room = total[1]
	}
	idx := make([]uint64, count+1)
	pos := make([]uint64, total[0]+1)
	sizes = make([]uint64, count)
	status := make([]int32, count)
	if err := hip(C.hipMemcpy(unsafe.Pointer(&idx[0]), dIdx, C.size_t(8*(count+1)), C.hipMemcpyDeviceToHost)); err != nil {
		return nil, nil, nil, err
	}
	if total[0] > 0 {
		if err := hip(C.hipMemcpy(unsafe.Pointer(&pos[0]), dPos, C.size_t(8*total[0]), C.hipMemcpyDeviceToHost)); err != nil {
			return nil, nil, nil, err
		}
	}
	if err := hip(C.hipMemcpy(unsafe.Pointer(&sizes[0]), dSize, C.size_t(8*count), C.hipMemcpyDeviceToHost)); err != nil {
		return nil, nil, nil, err
	}
	if err := hip(C.hipMemcpy(unsafe.Pointer(&status[0]), dStatus, C.size_t(4*count), C.hipMemcpyDeviceToHost)); err != nil {
		return nil, nil, nil, err
	}
	breaks = make([][]uint64, count)
	errs = make([]error, count)
	for k := range streams {
		if idx[k] > idx[k+1] || idx[k+1] > total[0] {
			return nil, nil, nil, ErrDevice // (never: brk_idx is an exclusive scan that ends at the Breaks found)
		}
		breaks[k] = pos[idx[k]:idx[k+1]:idx[k+1]]
		if status[k] != 0 {
			errs[k] = toErr(C.int(status[k]), 0)
		}
	}
	return breaks, sizes, errs, nil
}

// SelectSegmentsRoute sets the route of later segment queries (ez_select_segments_route): 'p' the
// parts route at any stream length, 'v' never the parts route, 0 automatic.  Tests and A/B only.
func SelectSegmentsRoute(kind int) error {
	if st := C.ez_select_segments_route(C.int(kind)); st != C.EZ_OK {
		return toErr(st, 0)
	}
	return nil
}

// SegmentsPartsLast reports, of the last direct segment query or size query of this process,
// whichever came later (ez_segments_parts_last): parts walked in the parts route's first pass,
// records taken as they stood, parts walked again, parts filled (none by the size query's stage).
// All zero where the route did not run.
func SegmentsPartsLast() ([4]uint64, error) {
	var counts [4]uint64
	if st := C.ez_segments_parts_last((*C.uint64_t)(unsafe.Pointer(&counts[0]))); st != C.EZ_OK {
		return counts, toErr(st, 0)
	}
	return counts, nil
}

// DecompressBatchSized decodes independent streams whose decoded lengths the caller does not know, on
// the GPU: ez_decompressed_size_batch sizes them, the sizes and the count of concatenated streams
// that K2g's walk sized behind the fast kernels (ez_decompressed_size_segs_last) come back, the slots
// are laid out from the sizes (each rounded up to 16 bytes), and the decode is
// ez_decompress_batch_segmented's where that count is not zero, so that the segments of such streams
// take the fast decoders too, else ez_decompress_batch's with the largest slot and the extents as its
// hints.  The result for streams[k] is what NewReaderBytes(streams[k]) read to EOF produces, with
// the Reader's error in errs[k].  The streams are staged into device memory and the calls run on the
// null stream; every HIP call's result is checked before anything is used.
func DecompressBatchSized(streams [][]byte, blockSizeLimit int) ([][]byte, []error, error) {
	count := len(streams)
	if count == 0 {
		return nil, nil, nil
	}
	inOff := make([]uint64, count+1)
	maxLen := 0
	for k, s := range streams {
		inOff[k+1] = inOff[k] + uint64(len(s))
		if len(s) > maxLen {
			maxLen = len(s)
		}
	}
	host := make([]byte, 0, inOff[count])
	for _, s := range streams {
		host = append(host, s...)
	}
	var dIn, dOut, dInOff, dOutOff, dSize, dStatus, dWork unsafe.Pointer
	defer func() {
		for _, p := range []unsafe.Pointer{dIn, dOut, dInOff, dOutOff, dSize, dStatus, dWork} {
			if p != nil {
				C.hipFree(p)
			}
		}
	}()
	// every HIP call's result is checked: a failed copy must never hand back stale bytes as success
	hip := func(r C.hipError_t) error {
		if r != C.hipSuccess {
			return ErrDevice
		}
		return nil
	}
	for _, a := range []struct {
		p *unsafe.Pointer
		n uint64
	}{{&dIn, inOff[count]}, {&dInOff, 8 * uint64(count+1)}, {&dOutOff, 8 * uint64(count+1)}, {&dSize, 8 * uint64(count)},
		{&dStatus, 4 * uint64(count)}, {&dWork, uint64(C.ez_decompress_workspace(C.uint64_t(count)))}} {
		if err := hip(C.hipMalloc(a.p, C.size_t(a.n+16))); err != nil {
			return nil, nil, err
		}
	}
	if len(host) > 0 {
		if err := hip(C.hipMemcpy(dIn, unsafe.Pointer(&host[0]), C.size_t(len(host)), C.hipMemcpyHostToDevice)); err != nil {
			return nil, nil, err
		}
	}
	if err := hip(C.hipMemcpy(dInOff, unsafe.Pointer(&inOff[0]), C.size_t(8*(count+1)), C.hipMemcpyHostToDevice)); err != nil {
		return nil, nil, err
	}
	b := C.ez_batch{
		in: (*C.uint8_t)(dIn), in_off: (*C.uint64_t)(dInOff), out_size: (*C.uint64_t)(dSize), status: (*C.int32_t)(dStatus),
		count: C.uint64_t(count), max_len: C.uint64_t(maxLen),
	}
	if st := C.ez_decompressed_size_batch(C.int64_t(blockSizeLimit), &b, dWork, nil); st != C.EZ_OK {
		return nil, nil, toErr(st, 0)
	}
	size := make([]uint64, count)
	// (hipMemcpy to host waits for the query's kernels on the null stream, and reports their faults)
	if err := hip(C.hipMemcpy(unsafe.Pointer(&size[0]), dSize, C.size_t(8*count), C.hipMemcpyDeviceToHost)); err != nil {
		return nil, nil, err
	}
	var counts [3]uint64
	if st := C.ez_decompressed_size_segs_last(dWork, C.uint64_t(count), (*C.uint64_t)(unsafe.Pointer(&counts[0]))); st != C.EZ_OK {
		return nil, nil, toErr(st, 0)
	}
	outOff := make([]uint64, count+1)
	largest := uint64(0)
	for k := range streams {
		slot := (size[k] + 15) &^ 15
		outOff[k+1] = outOff[k] + slot
		if slot > largest {
			largest = slot
		}
	}
	if err := hip(C.hipMalloc(&dOut, C.size_t(outOff[count]+16))); err != nil {
		return nil, nil, err
	}
	if err := hip(C.hipMemcpy(dOutOff, unsafe.Pointer(&outOff[0]), C.size_t(8*(count+1)), C.hipMemcpyHostToDevice)); err != nil {
		return nil, nil, err
	}
	b.out = (*C.uint8_t)(dOut)
	b.out_off = (*C.uint64_t)(dOutOff)
	b.max_len = C.uint64_t(largest) // (decode: the largest output slot)
	b.in_bytes = C.uint64_t(inOff[count])
	b.out_bytes = C.uint64_t(outOff[count])
	var st C.int
	if counts[1] != 0 {
		st = C.ez_decompress_batch_segmented(C.int64_t(blockSizeLimit), &b, nil, nil)
	} else {
		st = C.ez_decompress_batch(C.int64_t(blockSizeLimit), &b, dWork, nil)
	}
	if st != C.EZ_OK {
		return nil, nil, toErr(st, 0)
	}
	out := make([]byte, outOff[count]+1)
	status := make([]int32, count)
	if outOff[count] > 0 {
		if err := hip(C.hipMemcpy(unsafe.Pointer(&out[0]), dOut, C.size_t(outOff[count]), C.hipMemcpyDeviceToHost)); err != nil {
			return nil, nil, err
		}
	}
	if err := hip(C.hipMemcpy(unsafe.Pointer(&size[0]), dSize, C.size_t(8*count), C.hipMemcpyDeviceToHost)); err != nil {
		return nil, nil, err
	}
	if err := hip(C.hipMemcpy(unsafe.Pointer(&status[0]), dStatus, C.size_t(4*count), C.hipMemcpyDeviceToHost)); err != nil {
		return nil, nil, err
	}
	res := make([][]byte, count)
	errs := make([]error, count)
	for k := range streams {
		if size[k] > outOff[k+1]-outOff[k] {
			return nil, nil, ErrDevice // (never: a size is at most its slot)
		}
		res[k] = out[outOff[k] : outOff[k]+size[k] : outOff[k]+size[k]]
		if status[k] != 0 {
			errs[k] = toErr(C.int(status[k]), 0)
		}
	}
	return res, errs, nil
}
