/*
 * leopard_amd.h -- MI355X-specific extensions of the Leopard C ABI.
 *
 * None of these is needed for drop-in use (include/leopard.h is the contract);
 * they let a GPU-resident caller avoid the synchronous host-memory semantics of
 * the reference (leopard.h:180-234 return only when results are written).
 */
#ifndef LEOPARD_AMD_EXT_H
#define LEOPARD_AMD_EXT_H

#include "leopard.h"

#ifdef __cplusplus
extern "C" {
#endif

/* HIP stream used by the calling thread's leo_encode/leo_decode on device
 * memory (a hipStream_t passed as void*; NULL = the legacy default stream).
 * Per thread. */
LEO_EXPORT void leo_amd_set_stream(void* hip_stream);

/* Scratch: the library keeps per (calling thread, device, stream) scratch --
 * a device arena, pinned staging, and for host-memory calls a pinned ring with
 * two streams -- and keeps at most 8 of them per thread (least recently used
 * freed first).  A thread's scratch is freed when the thread exits.  This call
 * frees the calling thread's scratch for `hip_stream` on every device, after
 * the work this library queued on that stream has finished; call it before
 * destroying a stream used with leo_amd_set_stream.  (void*)-1 frees the
 * calling thread's scratch of every stream. */
LEO_EXPORT void leo_amd_release_stream(void* hip_stream);

/* 1: device-resident calls return after enqueueing work on the stream (the
 * caller orders later reads on that stream).  0 (default): every call
 * synchronises, like the reference.  Host-memory calls are always synchronous.
 * Per thread. */
LEO_EXPORT void leo_amd_set_async(int async_enable);

/* Device ordinal the calling thread's calls run on (default: the current HIP
 * device at call time).  -1 restores the default.  Per thread. */
LEO_EXPORT void leo_amd_set_device(int device);

/* Host-memory calls of the calling thread split their columns into `ranges`
 * 64-byte-aligned ranges, range i coded on device i % device_count by its own
 * worker thread over that device's PCIe link; the call returns when all are
 * done.  -1 = one range per device; 0 = the LEO_AMD_FANOUT environment value
 * (default 1, no split).  At most one range per 4 KiB of columns.  Device
 * pointers are not affected.  Per thread. */
LEO_EXPORT void leo_amd_set_fanout(int ranges);

/* Encode/decode a column range of every piece: identical to leo_encode /
 * leo_decode over bytes [byte_offset, byte_offset + slice_bytes) of each
 * piece (both multiples of 64).  This is how independent GPUs shard one object
 * by 64-byte column blocks without any collective (each GPU owns a slice). */
LEO_EXPORT LeopardResult leo_amd_encode_slice(
    uint64_t buffer_bytes, uint64_t byte_offset, uint64_t slice_bytes,
    unsigned original_count, unsigned recovery_count, unsigned work_count,
    const void* const* const original_data, void** work_data);

LEO_EXPORT LeopardResult leo_amd_decode_slice(
    uint64_t buffer_bytes, uint64_t byte_offset, uint64_t slice_bytes,
    unsigned original_count, unsigned recovery_count, unsigned work_count,
    const void* const* const original_data, const void* const* const recovery_data,
    void** work_data);

/* Batches: object_count independent objects of one shape (same buffer_bytes,
 * counts and work_count), each with exactly the semantics of one leo_encode /
 * leo_decode call; original_data[o], recovery_data[o], work_data[o] are object
 * o's pointer arrays.  Every object is validated first: the first failing
 * object's result is returned and nothing runs.  Device-resident GF(2^8)
 * objects (n <= 256) on one device are coded by ONE kernel launch over every
 * object's columns -- a single 64 KiB-piece object gives each CU one
 * workgroup, a batch fills the GPU; other batches run object by object.
 * Decoding objects may have different erasure patterns. */
LEO_EXPORT LeopardResult leo_amd_encode_batch(
    unsigned object_count, uint64_t buffer_bytes, unsigned original_count, unsigned recovery_count,
    unsigned work_count, const void* const* const* original_data, void** const* work_data);

LEO_EXPORT LeopardResult leo_amd_decode_batch(
    unsigned object_count, uint64_t buffer_bytes, unsigned original_count, unsigned recovery_count,
    unsigned work_count, const void* const* const* original_data, const void* const* const* recovery_data,
    void** const* work_data);

/* In-place recovery update from original-piece deltas (the parity-delta
 * update of a partial-stripe write).  The code is linear in every byte column:
 * encode(D ^ delta) == encode(D) ^ encode(delta), so when a few originals
 * change, the recovery pieces change by a sum over the changed pieces only,
 * and the unchanged originals are not needed.
 *
 * recovery_data[j] ^= XOR_t G[j][changed_index[t]] * delta_data[t], j < recovery_count, in place.
 * If recovery_data held leo_encode's output for originals D, it afterwards holds, bit for bit,
 * leo_encode's output for D with D[changed_index[t]] ^= delta_data[t].
 *
 * delta_data[t] is new piece XOR old piece of original changed_index[t]
 * (buffer_bytes bytes, read only).  At most LEO_AMD_UPDATE_MAX_CHANGED pieces
 * a call; a caller with more calls again or re-encodes.  All delta and
 * recovery pieces are of one kind: device memory (updated on the calling
 * thread's stream, honouring leo_amd_set_stream / set_async / set_device) or
 * host memory (registered ranges in place, pageable memory staged; the call
 * returns when the results are in host memory).  Deltas must not overlap
 * recovery pieces (not checked).
 *
 * Results, in this order, all decided before any GPU work:
 * Leopard_InvalidSize (buffer_bytes 0 or not a multiple of 64; slice form:
 * the slice checks of leo_amd_encode_slice); Leopard_InvalidCounts
 * (recovery_count 0 or > original_count, changed_count >
 * LEO_AMD_UPDATE_MAX_CHANGED); changed_count == 0 returns Leopard_Success and
 * touches nothing; Leopard_InvalidInput (a NULL array, a NULL delta_data[t] or
 * recovery_data[j], an index >= original_count, a repeated index;
 * leo_amd_last_error() names the position); Leopard_CallInitialize;
 * Leopard_TooMuchData (codeword length above 65536).
 *
 * The coefficients G[j][i] come from the library's own encoder and are cached
 * per device by (original_count, recovery_count, index), up to
 * LEO_AMD_UPDATE_CACHE_KB KiB (environment, read once; default 65536; 0 = no
 * caching).  Past that bound a call still succeeds: it builds the columns it
 * needs in scratch of its own. */
#define LEO_AMD_UPDATE_MAX_CHANGED 32

LEO_EXPORT LeopardResult leo_amd_update(
    uint64_t buffer_bytes, unsigned original_count, unsigned recovery_count,
    unsigned changed_count, const unsigned* changed_index,
    const void* const* delta_data, void** recovery_data);

/* The same over bytes [byte_offset, byte_offset + slice_bytes) of each piece. */
LEO_EXPORT LeopardResult leo_amd_update_slice(
    uint64_t buffer_bytes, uint64_t byte_offset, uint64_t slice_bytes,
    unsigned original_count, unsigned recovery_count,
    unsigned changed_count, const unsigned* changed_index,
    const void* const* delta_data, void** recovery_data);

/* Rebuild: regenerate every piece a failed node held, lost originals and lost
 * recovery pieces alike, in the decode pass.  The decode transform is
 * symmetric in the codeword positions: after it, the erased symbol of any
 * erased position is at hand, a recovery position as well as an original one,
 * so lost recovery pieces need no second pass over the originals (leo_decode
 * followed by a full leo_encode).
 *
 * original_data[i] == NULL marks a lost original; it is written to
 * work_data[i].  work_data[i] of a received original is neither read nor
 * written and may be NULL: unlike leo_decode, repair writes lost pieces only
 * and copies nothing when no original is lost.
 * recovery_data[j] == NULL marks a lost recovery piece.  It is requested when
 * recovery_out[j] != NULL, and only then is it written; a NULL recovery_out[j]
 * of a lost piece means "not wanted" (only one node's pieces are being
 * rebuilt).  recovery_out[j] of a received piece is ignored and never written.
 *
 * For consistent input (the received pieces come from one leo_encode codeword)
 * every written work_data[i] equals the original and every written
 * recovery_out[j] equals leo_encode's recovery piece j, bit for bit.  For
 * inconsistent input the lost originals are still bit-identical to
 * leo_decode's output; the rebuilt recovery pieces are unspecified.
 *
 * work_count is as for leo_decode (leo_decode_work_count) and checked the same
 * way.  All pieces are of one kind: device memory (on the calling thread's
 * stream, honouring leo_amd_set_stream / set_async / set_device) or host
 * memory (registered ranges in place, pageable memory staged: inputs are the
 * received pieces, outputs the lost originals, then the requested recovery
 * pieces; the call returns when the results are in host memory; the columns
 * fan out as for leo_decode, leo_amd_set_fanout).  Outputs must not overlap
 * inputs or each other (not checked).
 *
 * Results, in this order: Leopard_InvalidSize (slice form: the slice checks of
 * leo_amd_decode_slice); Leopard_InvalidCounts (recovery_count 0 or >
 * original_count); Leopard_InvalidInput for a NULL array (leo_amd_last_error()
 * names it); Leopard_CallInitialize; Leopard_NeedMoreData (fewer recovery
 * pieces received than originals lost, as leo_decode: lost originals + lost
 * recovery > recovery_count); on the general path (original_count > 1,
 * recovery_count > 1) Leopard_InvalidCounts for work_count != n, then
 * Leopard_TooMuchData for n > 65536; Leopard_InvalidInput for a lost original
 * whose work_data[i] is NULL.  Nothing lost or nothing requested returns
 * Leopard_Success and touches nothing.
 *
 * original_count == 1: every piece is a copy of the one original (from the
 * original if received, else from the last received recovery piece).
 * recovery_count == 1: a lost recovery_data[0] is the XOR of all originals.
 *
 * LEO_AMD_REPAIR_COMPOSE=1 (environment, read once) forces the composition the
 * call replaces -- the decoder, then the encoder over received and rebuilt
 * originals with unrequested rows in scratch -- for comparison. */
LEO_EXPORT LeopardResult leo_amd_repair(
    uint64_t buffer_bytes, unsigned original_count, unsigned recovery_count, unsigned work_count,
    const void* const* original_data, const void* const* recovery_data,
    void** work_data, void** recovery_out);

/* The same over bytes [byte_offset, byte_offset + slice_bytes) of each piece. */
LEO_EXPORT LeopardResult leo_amd_repair_slice(
    uint64_t buffer_bytes, uint64_t byte_offset, uint64_t slice_bytes,
    unsigned original_count, unsigned recovery_count, unsigned work_count,
    const void* const* original_data, const void* const* recovery_data,
    void** work_data, void** recovery_out);

/* object_count objects of one shape, each with the semantics of one
 * leo_amd_repair call; objects may differ in pattern and in what they request.
 * Every object is validated first: the first failing object's result is
 * returned and nothing runs.  Device-resident GF(2^8) objects (n <= 256) on one
 * device run as one launch per 256 objects; other batches object by object. */
LEO_EXPORT LeopardResult leo_amd_repair_batch(
    unsigned object_count, uint64_t buffer_bytes, unsigned original_count, unsigned recovery_count,
    unsigned work_count, const void* const* const* original_data, const void* const* const* recovery_data,
    void** const* work_data, void** const* recovery_out);

/* Scrub: check that stored recovery pieces still belong to the originals,
 * without writing any piece.  A store proves periodically that the K originals
 * and the R recovery pieces it holds still form one codeword; this is
 * leo_encode into scratch plus a compare, inside one call that keeps the
 * scratch bounded and reports one bit per recovery piece.
 *
 * Every original is needed: original_data[i] == NULL is Leopard_InvalidInput
 * (leo_amd_last_error() names i).  recovery_data[j] == NULL means "piece j is
 * not at hand, do not check it".  A checked piece j mismatches when any byte of
 * recovery_data[j] differs from what leo_encode of these originals writes to
 * work_data[j] (slice form: any byte of the slice's columns; original_count ==
 * 1: every piece is compared with the original; recovery_count == 1: with the
 * XOR of all originals).
 *
 * *mismatch_count (required) receives the number of checked pieces that
 * mismatch.  mismatch may be NULL; otherwise it is (recovery_count + 31) / 32
 * words of host memory: bit j (bit j % 32 of word j / 32) is set exactly for
 * the mismatching checked pieces, every other bit is cleared.  How to read it:
 * one bit set -- that recovery piece is bad; every checked bit set -- an
 * original is bad (any change of an original changes every recovery piece).
 * Leopard_Success means "the check ran"; the verdict is in the outputs, which
 * are written only on Leopard_Success.  With no piece to check the call
 * returns Leopard_Success with a zero count and touches nothing on the GPU.
 *
 * The reports are host memory: the call returns when they are filled in, in
 * async mode (leo_amd_set_async) too.  It runs on the calling thread's stream
 * and device (leo_amd_set_stream / set_device), as the other extensions.
 * All pieces are of one kind: device memory, or host memory (registered ranges
 * are read in place, pageable memory is staged up; nothing is copied back).
 * A host-memory call runs on one device: its columns are not fanned out
 * (leo_amd_set_fanout does not apply).
 *
 * Results, in this order, all decided before any GPU work:
 * Leopard_InvalidSize (slice form: the slice checks of leo_amd_encode_slice);
 * Leopard_InvalidCounts (recovery_count 0 or > original_count);
 * Leopard_InvalidInput (original_data, recovery_data or mismatch_count NULL, or
 * a NULL original); Leopard_CallInitialize; Leopard_TooMuchData (as leo_encode).
 *
 * A call runs the verify form of the kernel with which leo_encode of the same
 * shape writes the recovery pieces: it loads the stored recovery dwords where
 * the encoder would store, compares, and ORs one bit per differing piece into
 * a report in device memory; a clean stripe writes nothing.  The shapes without
 * such a form (the GF(2^8) matrix path, the GF(2^16) chunk-parallel encoder of
 * small pieces, original_count == 1, recovery_count == 1) run the composed route:
 * the encoder into workspace scratch, a column slice at a time, then a compare
 * kernel with the same report.  LEO_AMD_VERIFY_COMPOSE=1 (environment, read
 * once) forces the composed route everywhere, for comparison. */
LEO_EXPORT LeopardResult leo_amd_verify(
    uint64_t buffer_bytes, unsigned original_count, unsigned recovery_count,
    const void* const* original_data, const void* const* recovery_data,
    uint32_t* mismatch, unsigned* mismatch_count);

/* The same over bytes [byte_offset, byte_offset + slice_bytes) of each piece:
 * bisects the bad column range of a large piece. */
LEO_EXPORT LeopardResult leo_amd_verify_slice(
    uint64_t buffer_bytes, uint64_t byte_offset, uint64_t slice_bytes,
    unsigned original_count, unsigned recovery_count,
    const void* const* original_data, const void* const* recovery_data,
    uint32_t* mismatch, unsigned* mismatch_count);

/* object_count objects of one shape, each with the semantics of one
 * leo_amd_verify call: mismatch_count is an array of object_count entries and
 * mismatch, if given, object_count rows of (recovery_count + 31) / 32 words.
 * Every object is validated first: the first failing object's result is
 * returned and nothing runs.  Device-resident objects on one device run as
 * batch launches (the batch encoder's routes, then one compare launch over
 * every object's pieces); other batches object by object. */
LEO_EXPORT LeopardResult leo_amd_verify_batch(
    unsigned object_count, uint64_t buffer_bytes, unsigned original_count, unsigned recovery_count,
    const void* const* const* original_data, const void* const* const* recovery_data,
    uint32_t* mismatch, unsigned* mismatch_count);

/* Caller-registered host memory: pins [ptr, ptr + bytes) and maps it for
 * every device.  leo_encode / leo_decode calls whose host pieces all lie in
 * registered ranges run the kernels on them in place (reads and writes over
 * PCIe, no staging copies); other host pieces go through the pinned staging
 * pipeline.  The range must stay allocated until leo_amd_unregister_host(ptr)
 * (the contract of hipHostRegister and RDMA memory registration).
 * Returns Leopard_Platform when the runtime refuses the registration. */
LEO_EXPORT LeopardResult leo_amd_register_host(void* ptr, uint64_t bytes);
LEO_EXPORT LeopardResult leo_amd_unregister_host(void* ptr);

/* Number of HIP devices usable by the library (0 when none / not gfx950). */
LEO_EXPORT int leo_amd_device_count(void);

/* Host-side tables, for conformance tests (no GPU needed).  field: 8 or 16.
 * which: 0 = log (Cantor basis), 1 = exp, 2 = FFT skew (as logs), 3 = LogWalsh.
 * Copies up to `capacity` uint16 entries into out; returns the table length,
 * or a negative LeopardResult. */
LEO_EXPORT int leo_amd_table(int field, int which, uint16_t* out, unsigned capacity);

/* Human-readable description of the last error on the calling thread. */
LEO_EXPORT const char* leo_amd_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* LEOPARD_AMD_EXT_H */
