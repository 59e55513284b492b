/*
 * lzf_gpu.h -- batched, device-resident LZF API of liblzf_hip.so.
 *
 * The reference has no batch entry point: it calls lzf_compress once per
 * SET/MSET key (src/query.c:391, reached from src/query.c:453 and :500) and
 * lzf_decompress once per GET/MGET item (src/net.c:1229, src/net.c:1309).
 * These calls take a whole batch of independent values at once; each value
 * gets exactly the single-call semantics of src/lzf_c.c / src/lzf_d.c
 * (results bit-identical to the reference, per-value return value and
 * errno), so the single-call drop-in in lzf.h is a batch of one.
 *
 * Layout: values are addressed by (offset, length) pairs into one byte
 * arena per direction.  Every pointer passed to lzf_gpu_* is DEVICE memory
 * (hipMalloc'd, or torch CUDA tensors); `stream` is a hipStream_t (NULL =
 * the legacy default stream).  Calls are asynchronous on `stream`.
 *
 * Return value of every call: LZF_GPU_OK or a negative LZF_GPU_E* code
 * (the launch was not made).  Failures are returned, never aborted on.
 *
 * Bounds: a value longer than max_in_len (compress) or with an out_cap past
 * max_out_cap (decompress) -- a caller that under-states the bound -- gets
 * out_len 0 (and err EINVAL on decompress); nothing outside its own output
 * range is written.
 */
#ifndef LZF_GPU_H
#define LZF_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LZF_GPU_OK          0
#define LZF_GPU_EARG       -1   /* bad argument (NULL pointer, count 0 ...) */
#define LZF_GPU_ELAUNCH    -2   /* HIP launch / copy failed */
#define LZF_GPU_ENODEV     -3   /* no usable gfx950 device */
#define LZF_GPU_ENOMEM     -4   /* device / pinned allocation failed */

/* Largest value the batch kernels take in one piece (bytes).  Gibson's
 * default max_value_size is far below it (src/default.h:52) and the shipped
 * config's 2 MiB (debian/etc/gibson/gibson.conf:33) too. */
#define LZF_GPU_MAX_VALUE  (64u << 20)

/*
 * Compress `count` values.  Value i is in[in_off[i] .. +in_len[i]); its
 * stream is written to out[out_off[i] .. +out_cap[i]) and its length to
 * out_len[i] (0 = does not fit, exactly when src/lzf_c.c returns 0; the
 * bytes at out then are unspecified, and nothing is ever written at or past
 * out_cap[i]).  max_in_len is an upper bound on every in_len[i] (selects the
 * kernel's LDS plan without reading device memory); max_in_len 0 declares an
 * all-empty batch (every out_len 0, src/lzf_c.c:131).
 * The server policy of src/query.c:385 is out_cap[i] = in_len[i] - 4.
 */
int lzf_gpu_compress_batch(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                           uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                           uint32_t *out_len, uint32_t count, uint32_t max_in_len,
                           void *stream);

/*
 * Decompress `count` streams.  Stream i is in[in_off[i] .. +in_len[i]);
 * the decoded bytes go to out[out_off[i] .. +out_cap[i]); out_len[i] gets
 * the decoded length or 0, err[i] gets 0, E2BIG or EINVAL exactly as the
 * reference sets errno (src/lzf_d.c:72-131).  As in the reference, a stream
 * with in_len 0 still reads its first control byte, so in[in_off[i]] must be
 * readable.  max_out_cap bounds every out_cap[i].
 */
int lzf_gpu_decompress_batch(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                             uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                             uint32_t *out_len, int32_t *err, uint32_t count,
                             uint32_t max_out_cap, void *stream);

/*
 * Mixed-size batches.
 *
 * The two calls above pick one kernel plan for the whole batch from its
 * bound, so one large value gives every value of the batch the plan (and the
 * compress scratch stride) of that size.  The mixed calls below sort the
 * values into size classes first and run every non-empty class as a batch of
 * its own, through the same routing, with the class's own largest length as
 * its bound.  Results are identical to the uniform calls', value by value.
 * Use them when a batch's sizes spread over more than one class (MSET / MGET
 * of arbitrary values); a batch of one size gains nothing and pays the
 * partition.
 *
 * Classes (lzf_gpu_size_class; the edges are those of the routing):
 *   compress, by in_len:    0: <= 4096   1: <= 8192   2: <= 16384
 *                           3: <= 65536  4: past 65536
 *   decompress, by out_cap: 0: <= 4096   1: <= 16384  2: past 16384
 * A value past the caller's bound (in_len > max_in_len, out_cap >
 * max_out_cap) is refused, reported as class LZF_GPU_NCLASS: out_len 0 (and
 * err EINVAL on decompress), nothing written to its slot -- the contract of
 * the uniform calls.
 */
#define LZF_GPU_NCLASS           5
#define LZF_GPU_KIND_COMPRESS    0
#define LZF_GPU_KIND_DECOMPRESS  1

/* The class of a length (pure host function; LZF_GPU_EARG for a bad kind). */
int lzf_gpu_size_class(uint32_t len, int kind);

/*
 * Stable partition of `count` lengths by class, on the device.  perm[k] is
 * the index of the k-th value in class-major order; inside a class the
 * original order is kept; values with len > bound come last.  class_count and
 * class_max have LZF_GPU_NCLASS + 1 entries each (the last: the refused
 * values): how many values a class holds and the largest length present in
 * it (0 for an empty class).  `work` is device scratch of
 * lzf_gpu_size_partition_work_size(count) bytes; every pointer is device
 * memory; asynchronous on `stream`.  count: anything up to 2^32 - 1.
 */
uint64_t lzf_gpu_size_partition_work_size(uint32_t count);
int lzf_gpu_size_partition(const uint32_t *len, uint32_t count, uint32_t bound, int kind,
                           uint32_t *perm, uint32_t *class_count, uint32_t *class_max,
                           void *work, void *stream);
/* The same partition in host memory; makes no HIP call. */
int lzf_host_size_partition(const uint32_t *len, uint32_t count, uint32_t bound, int kind,
                            uint32_t *perm, uint32_t *class_count, uint32_t *class_max);

/*
 * lzf_gpu_compress_batch / lzf_gpu_decompress_batch with per-class routing.
 * The arguments mean what they mean there; `work` is device scratch of
 * lzf_gpu_mixed_work_size(count) bytes that must stay valid until the
 * stream's work is done.
 *
 * THE ONE WAIT: unlike the uniform calls, a mixed call is not fully
 * asynchronous.  It enqueues the partition on `stream`, copies the 48 bytes
 * of class counts and maxima to pinned host memory and WAITS for that copy
 * (and so for everything enqueued on `stream` before it) -- the host needs
 * them to launch the class batches.  Everything after that is asynchronous
 * on `stream` as usual.  A mixed call therefore cannot be captured in a HIP
 * graph.
 *
 * Classes that the routing sends to window64 (no scratch, few waves) run on
 * a library-owned side stream per device, forked from and joined to `stream`
 * by events, beside the scratch-using classes, which run on `stream` one
 * after the other, largest class first.  A batch whose values all fall in
 * one class runs exactly one class batch and no side stream.
 */
uint64_t lzf_gpu_mixed_work_size(uint32_t count);
int lzf_gpu_compress_mixed(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                           uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                           uint32_t *out_len, uint32_t count, uint32_t max_in_len,
                           void *work, void *stream);
int lzf_gpu_decompress_mixed(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                             uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                             uint32_t *out_len, int32_t *err, uint32_t count,
                             uint32_t max_out_cap, void *work, void *stream);
/*
 * The plan of the calling thread's last mixed device call: for k < max (up
 * to LZF_GPU_NCLASS + 1), class_count[k], class_max[k] and route[k]:
 * 0 empty (or refused), and for compress 1 lane, 2 table, 3 window64 (4: a
 * diagnostic generation); for decompress 1 tokpar64, 2 tokpar64-far, 3 pipe.
 * Returns the number of class batches the call launched.
 */
int lzf_gpu_mixed_last_plan(uint32_t *class_count, uint32_t *class_max, int *route, int max);

/*
 * The host-memory batches (lzf_host_compress_batch / lzf_host_decompress_batch
 * below, same arguments, host pointers) with per-class routing: the lengths
 * are partitioned on the host (lzf_host_size_partition, no bound: nothing is
 * refused), and every non-empty class goes through the uniform host call as
 * one batch of class-contiguous descriptors -- registered or staged
 * pipelines, chunking, LZF_GPU_DEVICES and the split as they stand.
 * lzf_host_last_spread then describes the last class's call.
 */
int lzf_host_compress_mixed(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                            uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                            uint32_t *out_len, uint32_t count);
int lzf_host_decompress_mixed(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                              uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                              uint32_t *out_len, int32_t *err, uint32_t count);

/*
 * Decoded-size pre-pass: out_size[i] gets the length lzf_decompress would
 * return for stream i with out_len = out_limit (0 on failure) and err[i]
 * its errno (0, E2BIG or EINVAL in the reference's check order,
 * src/lzf_d.c:64-146); nothing is decoded.  For MGET items without an
 * original-length side-table entry: size them at out_limit = maxrequestsize
 * (src/net.c:1309-1315), then decode into exact slots (gb_mget_payload, or
 * val_len for lzf_gpu_kv_frame).  As for decompress, in[in_off[i]] must be
 * readable even when in_len[i] is 0.
 */
int lzf_gpu_decoded_size_batch(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                               uint32_t *out_size, int32_t *err, uint32_t count, uint32_t out_limit,
                               void *stream);
int lzf_host_decoded_size_batch(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                                uint32_t *out_size, int32_t *err, uint32_t count, uint32_t out_limit);

/*
 * Fill `count` values of n bytes each, value k at out[k*n], with synthetic
 * generator `kind` (gibson_amd/csrc/synth.h) at indices first + k*stride.
 * Bench/test data generation directly in HBM.
 */
int lzf_gpu_synth_fill(int kind, uint64_t seed, uint64_t first, uint64_t stride,
                       uint32_t count, uint32_t n, uint8_t *out, void *stream);

/*
 * Host-memory batch (the north star's PCIe-inclusive path): the same as the
 * device calls, but every pointer is host memory, and the call returns after
 * the results are back in host memory.
 *
 * Devices: with LZF_GPU_DEVICES set ("0,1,2,3", "all"; an index may repeat),
 * value i goes to entry i mod G of that list, each entry served by its own
 * worker thread (bound to its device's NUMA node), streams and staging; the
 * results land at index i.  A failure on any entry makes the call return
 * that entry's LZF_GPU_E* code.  Unset: the one device LZF_GPU_DEVICE
 * (default 0), on the calling thread.
 *
 * Moving bytes: when both arenas' spans lie in ranges given to
 * lzf_host_register, no CPU copies a value byte (the GPU and its DMA engines
 * move them; the bytes of an output slot past out_len[i] are then either
 * left as they were or zeroed -- never bytes of another value).  Otherwise
 * the library stages values through its own pinned buffers.  Results are
 * identical either way.
 *
 * LZF_GPU_SPLIT=block gives entry g a contiguous span of the values instead
 * of every G-th one (lzf_host_split_block below).
 */
int lzf_host_compress_batch(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                            uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                            uint32_t *out_len, uint32_t count);
int lzf_host_decompress_batch(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                              uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                              uint32_t *out_len, int32_t *err, uint32_t count);

/*
 * Register [ptr, ptr+len) of caller memory (an arena of request buffers, the
 * store's values) for the host-memory batches: page-locked and mapped into
 * every device of the plan (hipHostRegister, portable + mapped).  The range
 * must stay allocated until lzf_host_unregister(ptr).  Returns LZF_GPU_OK,
 * LZF_GPU_EARG (NULL, empty, or overlapping a registered range) or the HIP
 * failure's code.  Registration costs about 15 ms per GiB (measured).
 */
int lzf_host_register(const void *ptr, uint64_t len);
/* (LZF_GPU_ENODEV: some device of the plan gave no device address for the
 * range; it is then left unregistered.) */
int lzf_host_unregister(const void *ptr);

/*
 * The device plan of the host-memory calls: returns G, the number of
 * entries, and fills (for k < max) device[k] (HIP device index),
 * numa_node[k] (the device's node from sysfs, -1 unknown) and bound[k]
 * (1 when entry k's worker thread runs on that node's CPUs with its memory
 * preferred there).  A negative LZF_GPU_E* code when the plan is invalid.
 */
int lzf_gpu_device_plan(int *device, int *numa_node, int *bound, int max);
/* The calling thread's last host-memory call: values each plan entry took
 * and its wall time in ms (the per-device spread).  Returns G. */
int lzf_host_last_spread(uint32_t *values, double *ms, int max);
/* The partition rule: entry g of `groups` takes values first + k * stride,
 * k < the returned count (first = g, stride = groups): value i to entry
 * i mod G, the default. */
uint32_t lzf_host_split(uint32_t count, uint32_t groups, uint32_t g, uint32_t *first, uint32_t *stride);
/* The contiguous split (LZF_GPU_SPLIT=block): entry g takes the values
 * [first, first + returned count), first = floor(count * g / groups), so
 * every entry's share is one span of the caller's arena and its values keep
 * the registered path's DMA runs. */
uint32_t lzf_host_split_block(uint32_t count, uint32_t groups, uint32_t g, uint32_t *first);
/* The split the host-memory calls use: 0 round-robin (default), 1 block. */
int lzf_host_split_policy(void);
/* The LZF_GPU_DEVICES grammar ("all", or comma-separated indices below
 * `visible`): fills dev[] and returns the count, or a negative code. */
int lzf_gpu_parse_device_list(const char *spec, int visible, int *dev, int max);

/*
 * MGET / KEYS reply assembled on the device.
 *
 * Builds exactly the payload of gbClientEnqueueKeyValueSet
 * (src/net.c:1256-1342) -- u32 `elements`, then per item that is not
 * LZF_ENC_NULL: [u32 key size][key][u8 encoding][u32 value size][value],
 * little-endian, LZF items emitted as PLAIN with their decoded bytes -- and,
 * with reply_header != 0, the [i16 REPL_KVAL][u8 PLAIN][u32 size] reply
 * header of gbClientEnqueueData (src/net.c:1162-1205) in front.
 *
 * Item i: key keys[key_off[i] .. +key_len[i]); encoding enc[i]; stored
 * bytes vals[val_off[i] .. +val_size[i]) (the LZF stream for an LZF item,
 * the 8-byte little-endian number for a NUMBER item, src/net.c:1321-1329).
 * val_len[i] is the decoded length of an LZF item -- the original length
 * recorded at SET time (the side table of §8(f) rank 3); max_val_len bounds
 * it.  LZF items are decoded straight into the frame (no bounce buffer).
 *
 * frame must hold (reply_header ? 7 : 0) + max_response bytes.  On the
 * device, *frame_len receives the frame's byte count, or 0 when the payload
 * exceeds max_response (the reference's CHECK_SPACE, src/net.c:1272-1277)
 * or an LZF item did not decode to val_len[i].  `work` is device scratch of
 * lzf_gpu_kv_frame_work_size(count) bytes.
 */
#define LZF_ENC_PLAIN   0x00   /* GB_ENC_PLAIN,  src/net.h:274 */
#define LZF_ENC_LZF     0x01   /* GB_ENC_LZF,    src/net.h:276 */
#define LZF_ENC_NUMBER  0x02   /* GB_ENC_NUMBER, src/net.h:278 */
#define LZF_ENC_NULL    0xFF   /* expired / missing item: skipped (src/net.c:1287) */
#define LZF_REPL_KVAL   7      /* src/query.h:71 */

uint64_t lzf_gpu_kv_frame_work_size(uint32_t count);
int lzf_gpu_kv_frame(const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len,
                     const uint8_t *vals, const uint64_t *val_off, const uint32_t *val_size,
                     const uint8_t *enc, const uint32_t *val_len, uint32_t count,
                     uint32_t elements, uint32_t max_val_len, int reply_header,
                     uint8_t *frame, uint64_t max_response, uint64_t *frame_len, void *work,
                     void *stream);

/*
 * SET batch into a device-resident store (the write side of lzf_gpu_kv_frame).
 *
 * gbSingleSet for a whole batch, the values never leaving HBM: the store
 * decision (src/query.c:389-397), the dense copy into the store
 * (src/query.c:409) and the item's size and encoding (src/query.c:408-417).
 * Value i is in[in_off[i] .. +in_len[i]).  It is compressed iff
 * in_len[i] > compression (strict, src/query.c:389), with the reference's
 * out_len = vlen - 4 (for a value shorter than 4 bytes the wrapped size_t:
 * no limit, so a 1-byte value at compression 0 is stored LZF as 2 bytes).
 *   a stream:      enc[i] = LZF_ENC_LZF,   val_size[i] = the stream's length;
 *   no stream (0): enc[i] = LZF_ENC_PLAIN, val_size[i] = in_len[i], the input
 *                  bytes stored -- also for in_len[i] == 0 (size 0) and for a
 *                  value past max_in_len (a caller that under-states the bound).
 * The original length of an LZF item is in_len[i]: pass in_len to
 * lzf_gpu_kv_frame as val_len.
 *
 * The stored bytes are packed densely, in request order, from base =
 * *store_used: val_off[i] = base + the sizes before i (64-bit), at
 * store + val_off[i].  On success *store_used = base + the batch's bytes and
 * *status = LZF_STORE_OK, so consecutive calls on one stream append to one
 * arena.  The batch is refused as a whole when base + its bytes exceed
 * store_cap (LZF_STORE_FULL) or when the compress slots do not fit in
 * in_bytes + 8 * count bytes (LZF_STORE_EWORK: in_bytes, the caller's upper
 * bound on the sum of in_len, was under-stated).  Then *store_used is
 * unchanged, no byte of store is written, every enc[i] is LZF_ENC_NULL and
 * every val_size[i] is 0.
 *
 * Every pointer is device memory, store_used (one u64) and status (one u32)
 * included.  `work` is device scratch of lzf_gpu_set_store_work_size(count,
 * in_bytes) bytes that must stay valid until the stream's work is done.
 * Asynchronous on `stream`, with no host wait.  count: up to 2^32 - 1.
 */
#define LZF_STORE_OK     0
#define LZF_STORE_FULL   1   /* base + packed bytes > store_cap */
#define LZF_STORE_EWORK  2   /* in_bytes under-stated: the scratch slots do not fit in work */

uint64_t lzf_gpu_set_store_work_size(uint32_t count, uint64_t in_bytes);
int lzf_gpu_set_store(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                      uint32_t count, uint32_t max_in_len, uint64_t in_bytes, uint32_t compression,
                      uint8_t *store, uint64_t store_cap, uint64_t *store_used,
                      uint64_t *val_off, uint32_t *val_size, uint8_t *enc, uint32_t *status,
                      void *work, void *stream);
/* host, no HIP call: the STATS fold of src/query.c:400-405 over a batch's
 * results (host copies of enc, val_size and in_len as val_len), once per
 * value stored LZF, in index order -- what `count` gbSingleSet calls leave
 * in server->stats.compravg, double for double */
int lzf_host_store_stats(const uint8_t *enc, const uint32_t *val_size, const uint32_t *val_len,
                         uint32_t count, double *compravg, uint64_t *ncompressed);

/*
 * The device store's lifecycle: delete, TTL expiry, usage, compaction.
 *
 * The store is the three arrays lzf_gpu_set_store writes and lzf_gpu_kv_frame
 * reads -- val_off[count] (u64), val_size[count] (u32), enc[count] (u8) --
 * over an arena.  An item is dead once enc[i] == LZF_ENC_NULL; every other
 * item is live (PLAIN, LZF, and NUMBER with its 8 stored bytes).  Delete,
 * expire, usage and compact keep item indices: a key -> index map stays valid
 * across a compaction.  lzf_gpu_store_renumber is the one call that does not:
 * it gives the dead items' indices and key bytes back, and hands out the remap
 * from old to new indices.  Every pointer is device memory; every call
 * validates its arguments before any HIP call, is asynchronous on `stream`
 * and waits for nothing on the host, so SET, MGET, DEL / expire, compact and
 * SET again queue behind each other on one stream.
 */

/* DEL / overwrite: enc[idx[k]] = LZF_ENC_NULL for k < n.  An index >= count is
 * ignored; duplicates are fine; n == 0 does nothing.  val_off / val_size are
 * left as they are (usage and compact read them). */
int lzf_gpu_store_delete(const uint32_t *idx, uint32_t n, uint8_t *enc, uint32_t count, void *stream);

/* TTL sweep, the rule of gbIsNodeStillValid / gbIsItemStillValid
 * (src/query.c:186-189): item i expires iff ttl[i] > 0 and
 * now - item_time[i] >= ttl[i]; then enc[i] = LZF_ENC_NULL.  Items already
 * NULL are not counted.  *expired (one device u32) receives how many items
 * this call nulled. */
int lzf_gpu_store_expire(const int64_t *item_time, const int32_t *ttl, int64_t now,
                         uint8_t *enc, uint32_t count, uint32_t *expired, void *stream);

/* What a compaction would find, without moving anything: report[0] live items
 * (enc != LZF_ENC_NULL), [1] their bytes (the sum of val_size), [2] dead
 * items, [3] the bytes the dead items' val_size still name (0 after a
 * compaction, which sets a dead item's size to 0).  report: 4 device u64.
 * work: lzf_gpu_store_compact_work_size(count) bytes of device scratch. */
int lzf_gpu_store_usage(const uint32_t *val_size, const uint8_t *enc, uint32_t count,
                        uint64_t *report, void *work, void *stream);

/*
 * Compaction: a semispace collection from the arena src (src_cap bytes) into
 * a second arena dst (dst_cap bytes).  The stored bytes of every live item
 * are copied from src + val_off[i] and packed densely IN ITEM-INDEX ORDER from
 * base = *dst_used, whatever order the old offsets were in (after overwrites
 * they are not monotone in the index; the result is).  On success, for every
 * i, live or dead, val_off[i] = base + the sizes of the live items before i;
 * val_size[i] is unchanged for a live item and 0 for a dead one; enc is not
 * written; *dst_used = base + the live bytes; *status = LZF_STORE_OK.  These
 * are the invariants lzf_gpu_set_store leaves (monotone offsets, ties at dead
 * and zero-size items), so a later lzf_gpu_set_store appends to dst and
 * lzf_gpu_kv_frame reads it unchanged.  src is never written: the caller
 * swaps the arenas afterwards.
 *
 * The call is refused as a whole with LZF_STORE_ERANGE when a live item's
 * [val_off, val_off + val_size) leaves [0, src_cap), and otherwise with
 * LZF_STORE_FULL when base + the live bytes exceed dst_cap or wrap.  Then
 * val_off, val_size and *dst_used are unchanged, no byte of dst is written
 * and no byte of an out-of-range item is read.  report (4 device u64) is
 * filled either way, as lzf_gpu_store_usage fills it, from the values before
 * the call.
 *
 * LZF_GPU_EARG: a NULL pointer, count == 0, a zero cap, or [dst, dst + dst_cap)
 * overlapping [src, src + src_cap).  Compaction in place is not provided: it
 * would need workgroups to wait for one another, or a chunked bounce through
 * scratch; what is provided is the copy into a second arena.  `work`:
 * lzf_gpu_store_compact_work_size(count) bytes of device scratch that must
 * stay valid until the stream's work is done.  count: up to 2^32 - 1; all
 * byte arithmetic is 64-bit.
 */
#define LZF_STORE_ERANGE 3   /* a live item's [val_off, val_off + val_size) leaves [0, src_cap) */

uint64_t lzf_gpu_store_compact_work_size(uint32_t count);
int lzf_gpu_store_compact(const uint8_t *src, uint64_t src_cap,
                          uint64_t *val_off, uint32_t *val_size, const uint8_t *enc, uint32_t count,
                          uint8_t *dst, uint64_t dst_cap, uint64_t *dst_used,
                          uint64_t *report, uint32_t *status, void *work, void *stream);

/*
 * Renumbering: a semispace copy of the live items from one set of item arrays
 * (src, `count` items over the key arena src_keys) into a second set (dst,
 * dst_cap entries over the key arena dst_keys).  Compaction gives value bytes
 * back; this call gives item indices and key bytes back, which every overwrite,
 * DEL and expiry otherwise burns for good.  Nothing is done in place.
 *
 * Live items.  Item i is live iff src->enc[i] != LZF_ENC_NULL.  The TTL rule is
 * not applied here: run lzf_gpu_store_expire first.  The live item with the
 * r-th smallest index becomes item r of dst: the order is stable, so among
 * equal keys the highest index is the same item before and after.
 *
 * Copied members.  Every member is copied verbatim, val_off included: value
 * bytes do not move, and the order of val_off is whatever it was until
 * lzf_gpu_store_compact runs over the new arrays (before or after this call).
 *
 * Key bytes are packed densely in new-index order from base = *dst_keys_used:
 * dst->key_off[r] = base + the key lengths of the live items before r, the
 * bytes copied from src_keys + src->key_off[i].  Source offsets may be in any
 * order, with gaps, or shared by several items.  A live item with key_len == 0
 * is kept; it owns no bytes.
 *
 * The tail.  dst entries [live, dst_cap) become dead items: enc =
 * LZF_ENC_NULL, val_size = val_len = key_len = 0, the time, ttl, lock and
 * last_access members (where given) 0, and the offsets the end offsets, as
 * compaction leaves ties: key_off = the new *dst_keys_used, val_off = the
 * highest val_off + val_size of a live item (saturating; 0 without one).  A
 * caller that does not know `live` on the host yet can therefore go on calling
 * every operator with count = dst_cap.
 *
 * remap (count device u32, may be NULL): remap[i] = the new index of item i,
 * or 0xFFFFFFFF for a dead item.  report (4 device u64) is filled whether the
 * call is accepted or refused, from the values before the call: [0] live
 * items, [1] their key bytes, [2] dead items, [3] the key bytes that dead
 * items still name.  The host needs report[0] before its next
 * lzf_gpu_set_store, as that call's `first`; nothing else has to be read back.
 *
 * *status (one device u32): LZF_STORE_OK; LZF_STORE_ERANGE when a live item's
 * [key_off, key_off + key_len) leaves [0, src_keys_cap) (64-bit, wrap-safe; a
 * dead item's key is never read or judged); otherwise LZF_STORE_FULL when
 * live > dst_cap, or when base + the live key bytes exceed dst_keys_cap or
 * wrap.  A refusal is whole: no byte of any dst array, of dst_keys or of remap
 * is written and *dst_keys_used is unchanged.  On success *dst_keys_used =
 * base + the live key bytes.  src and src_keys are never written.
 *
 * LZF_GPU_EARG, before any HIP call: a NULL struct; NULL among the six
 * required members (val_off, val_size, enc, val_len, key_off, key_len), the
 * key arenas, dst_keys_used, report, status or work; an optional member that
 * is NULL in one of src / dst and not in the other; exactly one of item_time /
 * item_ttl; count == 0, dst_cap == 0 or a zero key cap; [dst_keys, +
 * dst_keys_cap) overlapping [src_keys, + src_keys_cap); a dst array that is
 * the same pointer as the matching src array.  count and dst_cap: up to
 * 2^32 - 1.  Asynchronous on `stream`, with no host wait.  `work`:
 * lzf_gpu_store_renumber_work_size(count) bytes of device scratch that must
 * stay valid until the stream's work is done.
 *
 * Limits: semispace only; a short key (below 256 bytes) is staged by one lane.
 */
typedef struct lzf_store_items {          /* device pointers */
    uint64_t *val_off;  uint32_t *val_size;  uint8_t *enc;  uint32_t *val_len;
    uint64_t *key_off;  uint32_t *key_len;
    int64_t  *item_time; int32_t *item_ttl;  /* both or neither */
    int64_t  *item_lock;                     /* optional */
    int64_t  *last_access;                   /* optional */
} lzf_store_items;

uint64_t lzf_gpu_store_renumber_work_size(uint32_t count);
int lzf_gpu_store_renumber(const lzf_store_items *src, uint32_t count,
                           const uint8_t *src_keys, uint64_t src_keys_cap,
                           const lzf_store_items *dst, uint32_t dst_cap,
                           uint8_t *dst_keys, uint64_t dst_keys_cap, uint64_t *dst_keys_used,
                           uint32_t *remap /* count u32, may be NULL */,
                           uint64_t *report /* 4 u64 */, uint32_t *status,
                           void *work, void *stream);

/* An index list made before a renumbering (a select's or a lookup's output
 * still in flight), translated in place: idx[k] = idx[k] < count ?
 * remap[idx[k]] : 0xFFFFFFFF, count being the renumbering's.  Duplicates are
 * fine.  LZF_GPU_EARG: a NULL pointer, n == 0, count == 0. */
int lzf_gpu_store_remap(uint32_t *idx, uint32_t n, const uint32_t *remap, uint32_t count, void *stream);

/*
 * Prefix operators over the device store: select, MGET, COUNT, MTTL.
 *
 * Every multi-key operator of the reference is tr_search over a prefix plus a
 * callback per item found (src/query.c:526, 620, 687, 1171).  Here the search
 * is lzf_gpu_store_select_prefix, which leaves an index list in device
 * memory, and the callbacks are the index-list operators below; MDEL is
 * lzf_gpu_store_count followed by lzf_gpu_store_delete over the same list
 * (count's result[0] is the reply of gbQueryMultiDelHandler).  Everything
 * queues on one stream with no host wait.
 *
 * The store's per-item arrays, all of `count` entries: val_off, val_size, enc
 * (lzf_gpu_set_store), val_len (the original lengths, in_len of the SET),
 * keys / key_off / key_len (as lzf_gpu_kv_frame takes them), item_time (i64)
 * and item_ttl (i32) (as lzf_gpu_store_expire takes them), and last_access
 * (i64, optional: NULL is not written).
 *
 * Index lists.  idx[n] (u32), n given by the host.  An entry >= count is
 * ignored by every operator, as by lzf_gpu_store_delete, so 0xFFFFFFFF pads a
 * list made on the device and no device-side length is needed.
 *
 * The validity rule, shared by the three operators (gbIsItemStillValid with
 * remove = 1, src/query.c:204-224).  An in-range entry i is
 *   dead     if enc[i] == LZF_ENC_NULL;
 *   expired  if item_ttl[i] > 0 && now - item_time[i] >= item_ttl[i]; the
 *            operator then sets enc[i] = LZF_ENC_NULL (the device tr_remove);
 *   valid    otherwise.
 * item_time and item_ttl may both be NULL (nothing expires); exactly one of
 * them NULL is LZF_GPU_EARG.
 *
 * Order.  lzf_gpu_store_select_prefix yields matches in ascending item
 * index; the reference's tr_search yields them in trie pre-order with the
 * children in creation order (src/trie.c:154-176).  COUNT, MTTL, MDEL and
 * every operator that passes limit = -1 and replies a number do not depend on
 * the order: select -> operator is exact for them.  MGET with a limit, and
 * the reply order of MGET and KEYS, do depend on it: for those the index
 * list comes from lzf_gpu_store_select_ordered, which yields the reference's
 * order and applies its limit, on the device.  The one limit left: a
 * renumbering forgets the dead items' keys, and with them which sibling came
 * first (see there).
 *
 * LZF_GPU_EARG: a NULL pointer (but the optional ones), count == 0, n == 0,
 * and what each call names.  count and n: up to 2^32 - 1; all byte arithmetic
 * is 64-bit.
 */

/* Item i matches iff enc[i] != LZF_ENC_NULL, key_len[i] >= prefix_len and its
 * first prefix_len key bytes equal prefix (device memory).  A key equal to the
 * prefix matches (tr_recurse calls the handler on the start node), and so does
 * an expired item (tr_search returns it; the consuming operator drops it).
 * result (2 device u32): [1] the number of matches, [0] min(matches, cap).
 * sel[0 .. result[0]) holds the matching indices in ascending order,
 * sel[result[0] .. cap) is filled with 0xFFFFFFFF.  prefix_len == 0 or
 * cap == 0: LZF_GPU_EARG.  work: lzf_gpu_store_select_work_size(count) bytes
 * of device scratch that must stay valid until the stream's work is done. */
uint64_t lzf_gpu_store_select_work_size(uint32_t count);
int lzf_gpu_store_select_prefix(const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len,
                                const uint8_t *enc, uint32_t count,
                                const uint8_t *prefix, uint32_t prefix_len,
                                uint32_t *sel, uint32_t cap, uint32_t *result /* 2 u32 */,
                                void *work, void *stream);

/*
 * The ordered prefix select: the live matches in the order of the reference's
 * tr_search (src/trie.c:154-176), cut to its limit (src/trie.c:162).
 *
 * The rule.  The reference never frees a trie node while it runs: tr_remove
 * clears `data` only and an overwriting tr_insert reuses the node, so a
 * node's place among its siblings is fixed by the first insert, ever, of a key
 * with that prefix.  Item indices are handed out in insert order and a dead
 * item (enc == LZF_ENC_NULL) keeps key_off / key_len and its key bytes until a
 * renumbering.  So, with birth(P) the smallest index in [0, count) whose key
 * starts with the byte string P, live or dead, and row(K) of a key K the
 * sequence birth(K[0..d)) for d = prefix_len + 1 .. len(K): the reference's
 * order of the live matches is the ascending lexicographic order of their
 * rows, a row that is a proper prefix of another first -- the key equal to
 * the prefix first of all, a key before its extensions.
 *
 * Candidates are the items i < count with key_len[i] >= prefix_len whose first
 * prefix_len key bytes equal prefix, whatever enc holds; matches are the live
 * candidates (enc[i] != LZF_ENC_NULL; an expired item matches, as in the
 * select above).  limit > 0 keeps the first `limit` matches, limit <= 0 all.
 * sel[0 .. result[0]) holds them in order, cut to limit and then to cap, and
 * sel[result[0] .. cap) is 0xFFFFFFFF.  Two live items with the same key --
 * a store kept by lzf_gpu_key_index_upsert never holds them -- come in
 * ascending index.
 *
 * result (5 device u64): [0] the entries written, [1] the live matches, [2]
 * the candidates, [3] the node words needed, the sum of key_len - prefix_len
 * over the candidates, [4] LZF_ORDER_OK or LZF_ORDER_EWORK: the candidates
 * exceed cand_cap or the node words exceed node_cap.  The call is then
 * refused whole: all of sel is 0xFFFFFFFF and result[0] = 0, while [1], [2]
 * and [3] hold what they always hold, so the host repeats the call with
 * cand_cap >= result[2] and node_cap >= result[3] (the pattern of
 * LZF_REPLY_TOO_BIG).
 *
 * work: lzf_gpu_store_select_ordered_work_size(count, cand_cap, node_cap,
 * cap) bytes of device scratch that must stay valid until the stream's work is
 * done; about 12 * count / 64 + 28 * cand_cap bytes and 20 to 36 bytes per
 * node word (a table of 64-bit words, a power of two of at least twice
 * node_cap, and the rows).  ~0 when the size does not fit 64 bits; the call is
 * then LZF_GPU_EARG.  Asynchronous on `stream` with no host wait; every
 * length the call produces lives in the work area.
 *
 * Stated limit.  After lzf_gpu_store_renumber the dead items' keys are gone:
 * the births are then those of a server into which the surviving items were
 * inserted in index order.  Keys with a NUL byte stay outside the model, as
 * for KEYS.
 *
 * LZF_GPU_EARG: a NULL pointer, count == 0, prefix_len == 0, cap == 0,
 * cand_cap == 0, node_cap == 0.
 *
 * lzf_host_store_select_ordered is the same rule over host arrays, written as
 * the trie itself: children in arrival order and a pre-order walk.
 */
#define LZF_ORDER_OK    0
#define LZF_ORDER_EWORK 1
uint64_t lzf_gpu_store_select_ordered_work_size(uint32_t count, uint32_t cand_cap, uint64_t node_cap, uint32_t cap);
int lzf_gpu_store_select_ordered(const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len,
                                 const uint8_t *enc, uint32_t count,
                                 const uint8_t *prefix, uint32_t prefix_len, int64_t limit,
                                 uint32_t cand_cap, uint64_t node_cap,
                                 uint32_t *sel, uint32_t cap, uint64_t *result /* 5 u64 */,
                                 void *work, void *stream);
int lzf_host_store_select_ordered(const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len,
                                  const uint8_t *enc, uint32_t count,
                                  const uint8_t *prefix, uint32_t prefix_len, int64_t limit,
                                  uint32_t cand_cap, uint64_t node_cap,
                                  uint32_t *sel, uint32_t cap, uint64_t *result /* 5 u64 */);

/*
 * MGET over an index list: what gbQueryMultiGetHandler does after tr_search
 * (src/query.c:688-706), for the entries of idx in list order.  Dead and
 * expired entries drop out, expired ones are nulled in enc, every valid entry
 * gets last_access[i] = now, and `found` is the number of valid entries.  The
 * payload of gbClientEnqueueKeyValueSet is then built over the valid entries
 * with elements = found, taken on the device: exactly the bytes
 * lzf_gpu_kv_frame writes for the same items in the same order, LZF items
 * decoded straight into the frame.
 *
 * result (4 device u64): [0] found, [1] the entries this call expired, [2] the
 * entries skipped as dead or out of range, [3] one of LZF_MGET_*.
 * *frame_len: the frame's byte count on LZF_MGET_OK, otherwise 0.  frame must
 * hold (reply_header ? 7 : 0) + max_response bytes; no byte at or past that
 * is ever written, and none at all on NOT_FOUND or TOO_BIG.  The nulling and
 * last_access happen whatever the status is, as in the reference, where the
 * validity pass runs before the reply is built.  A duplicated entry is treated
 * on its own each time, emitted twice and counted twice, judged on what enc
 * held before the call.  max_val_len bounds val_len of the LZF items
 * (above LZF_GPU_MAX_VALUE: LZF_GPU_EARG).  work:
 * lzf_gpu_store_mget_work_size(n) bytes of device scratch that must stay valid
 * until the stream's work is done.
 */
#define LZF_MGET_OK         0
#define LZF_MGET_NOT_FOUND  1   /* no valid item: the host replies REPL_ERR_NOT_FOUND (src/query.c:731-735) */
#define LZF_MGET_TOO_BIG    2   /* payload > max_response: CHECK_SPACE, src/net.c:1272-1277 */
#define LZF_MGET_EDECODE    3   /* an LZF item did not decode to val_len */

uint64_t lzf_gpu_store_mget_work_size(uint32_t n);
int lzf_gpu_store_mget(const uint32_t *idx, uint32_t n,
                       const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len,
                       const uint8_t *store, const uint64_t *val_off, const uint32_t *val_size,
                       uint8_t *enc, const uint32_t *val_len, uint32_t count,
                       const int64_t *item_time, const int32_t *item_ttl, int64_t now,
                       int64_t *last_access /* may be NULL */,
                       uint32_t max_val_len, int reply_header,
                       uint8_t *frame, uint64_t max_response, uint64_t *frame_len,
                       uint64_t *result /* 4 u64 */, void *work, void *stream);

/* COUNT, gbCountCallback (src/query.c:1139-1157): the validity rule over the
 * list, last_access[i] = now for the valid entries; result (2 device u64):
 * [0] the valid entries -- 0 is an ordinary result, the reference replies
 * REPL_VAL 0 -- and [1] the entries this call expired.  Entries should be
 * distinct, as a trie walk or a select yields them: a duplicate is counted
 * each time it is valid, and a duplicated expired entry is counted as expired
 * at least once. */
int lzf_gpu_store_count(const uint32_t *idx, uint32_t n, uint8_t *enc, uint32_t count,
                        const int64_t *item_time, const int32_t *item_ttl, int64_t now,
                        int64_t *last_access, uint64_t *result /* 2 u64: valid, expired */, void *stream);
/* MTTL, gbMultiTtlCallback (src/query.c:580-600): a valid entry gets
 * item_time[i] = last_access[i] = now and item_ttl[i] = ttl, which the caller
 * has clamped to maxitemttl.  The time arrays must not be NULL.  result
 * (2 device u64): [0] the entries changed, [1] the entries this call expired.
 * Entries must be distinct; a duplicate is memory-safe, its count unspecified. */
int lzf_gpu_store_mttl(const uint32_t *idx, uint32_t n, int32_t ttl, uint8_t *enc, uint32_t count,
                       int64_t *item_time, int32_t *item_ttl, int64_t now,
                       int64_t *last_access, uint64_t *result /* 2 u64: changed, expired */, void *stream);

/*
 * Locks, the lock-aware DEL and INC / DEC over an index list.
 *
 * The store has one more caller-owned per-item array, item_lock (i64[count],
 * the reference's time_t lock, src/net.h:295), which the caller zeroes for new
 * items as it owns item_time and item_ttl.  The lock rule (gbItemIsLocked,
 * src/query.c:171-178): item i is locked iff
 *   item_lock[i] == -1 || now - item_time[i] < item_lock[i]
 * with the subtraction in two's complement, as in the validity rule above.
 * The operators below are the callbacks of LOCK / MLOCK, UNLOCK / MUNLOCK,
 * DEL / MDEL and INC / DEC / MINC / MDEC applied to an index list; with
 * MGET, COUNT and MTTL they are the reference's operator table over the
 * device store.  Every pointer is device memory, every call validates its
 * arguments before any HIP call (LZF_GPU_EARG: a NULL pointer but the
 * optional ones, n == 0, count == 0, and what each call names), is
 * asynchronous on `stream` and waits for nothing on the host.  count and n:
 * up to 2^32 - 1, all byte arithmetic 64-bit.  An idx entry >= count is
 * ignored.  Nothing outside the sizes named is written.
 *
 * entry_status (n device bytes, optional: NULL is not written) receives one
 * LZF_ENT_* code per entry; the host derives the single-key replies from
 * entry 0 (REPL_OK, REPL_ERR_NOT_FOUND, REPL_ERR_LOCKED, REPL_ERR_NAN).
 * Entries should be distinct, as a select or a lookup of distinct keys yields
 * them; a duplicate is memory-safe, its counts and values unspecified.
 */
#define LZF_ENT_DONE       0   /* the operator applied */
#define LZF_ENT_DEAD       1   /* out of range, padding, or already LZF_ENC_NULL */
#define LZF_ENT_EXPIRED    2   /* expired: this call set enc[i] = LZF_ENC_NULL */
#define LZF_ENT_LOCKED     3   /* locked: untouched */
#define LZF_ENT_NAN        4   /* minc: the value is not a number */
#define LZF_ENT_CONVERTED  5   /* minc: a PLAIN item became a NUMBER item */
#define LZF_ENT_UNCHANGED  6   /* minc: an LZF item, counted but untouched */

/* LOCK / MLOCK, gbMultiLockCallback (src/query.c:1015-1036).  Per entry, in
 * this order: dead -> DEAD; expired -> EXPIRED and nulled; locked -> LOCKED,
 * nothing written; otherwise item_time[i] = last_access[i] = now and
 * item_lock[i] = lock_time -> DONE.  Writing item_time restarts the item's TTL
 * clock, as in the reference.  item_time, item_ttl and item_lock are required.
 * result (3 device u64): [0] locked by this call (the reply of
 * gbQueryMultiLockHandler), [1] expired, [2] refused as locked. */
int lzf_gpu_store_mlock(const uint32_t *idx, uint32_t n, int64_t lock_time, uint8_t *enc, uint32_t count,
                        int64_t *item_time, const int32_t *item_ttl, int64_t *item_lock, int64_t now,
                        int64_t *last_access /* may be NULL */, uint8_t *entry_status /* may be NULL */,
                        uint64_t *result /* 3 u64: locked now, expired, refused */, void *stream);
/* UNLOCK / MUNLOCK, gbMultiUnlockCallback (src/query.c:1097-1114): a valid
 * entry gets item_lock[i] = 0 and last_access[i] = now, locked or not ->
 * DONE; dead and expired entries as above.  item_time is read only.  result
 * (2 device u64): [0] found, [1] expired. */
int lzf_gpu_store_munlock(const uint32_t *idx, uint32_t n, uint8_t *enc, uint32_t count,
                          const int64_t *item_time, const int32_t *item_ttl, int64_t *item_lock, int64_t now,
                          int64_t *last_access /* may be NULL */, uint8_t *entry_status /* may be NULL */,
                          uint64_t *result /* 2 u64: found, expired */, void *stream);
/* The lock-aware DEL / MDEL, gbMultiDelCallback (src/query.c:778-800), the
 * one-launch form of lzf_gpu_store_count followed by lzf_gpu_store_delete for
 * a store that uses locks.  Per entry, in this order: dead -> DEAD; locked --
 * tested first, on an expired item too (:789) -> LOCKED, untouched; expired
 * -> EXPIRED, nulled, not counted; valid -> enc[i] = LZF_ENC_NULL, DONE.
 * last_access is not written.  item_time and item_ttl: both NULL (nothing
 * expires) or both given; item_lock may be NULL (nothing is locked) and needs
 * item_time otherwise.  result (3 device u64): [0] deleted (the reply of
 * gbQueryMultiDelHandler), [1] expired, [2] locked. */
int lzf_gpu_store_mdel(const uint32_t *idx, uint32_t n, uint8_t *enc, uint32_t count,
                       const int64_t *item_time, const int32_t *item_ttl, const int64_t *item_lock /* may be NULL */,
                       int64_t now, uint8_t *entry_status /* may be NULL */,
                       uint64_t *result /* 3 u64: deleted, expired, locked */, void *stream);

/*
 * INC / DEC / MINC / MDEC: value + delta for every entry of the list.
 *
 * single == 0, gbMultiIncDecCallback (src/query.c:898-940), per entry in this
 * order: dead -> DEAD; locked -> LOCKED, untouched; expired -> EXPIRED,
 * nulled.  A valid entry gets last_access[i] = now -- before the value test,
 * so a NAN entry gets it too -- and then, by its encoding:
 *   LZF_ENC_NUMBER  the 8 stored little-endian bytes at store + val_off[i]
 *                   become value + delta                      -> DONE;
 *   LZF_ENC_PLAIN   whose bytes parse by the rule below: the item becomes a
 *                   NUMBER item holding parsed + delta        -> CONVERTED;
 *                   that do not parse, or of size 0           -> NAN, unchanged
 *                   and not counted;
 *   anything else   (LZF) -> UNCHANGED, and counted as found: the callback
 *                   falls through to return 1 (:939).
 * single != 0, gbQueryIncDecHandler (src/query.c:853-886): validity is tested
 * before the lock, so a locked and expired entry is EXPIRED and nulled, and an
 * LZF item is NAN.  Creating the item of a missing key (:842-851) is not
 * modelled: the entry reports DEAD and the host SETs 1.
 *
 * The parse rule (gbQueryParseLong, src/query.c:39-76): a first byte '0'
 * yields 0 whatever follows; a leading '-' negates, and a lone "-" yields 0;
 * every remaining byte must be '0'..'9' ("+5" and " 5" are not numbers);
 * there is no length limit, n = n * 10 + d accumulates modulo 2^64 -- what
 * the reference's x86-64 build computes where C leaves signed overflow
 * undefined -- and + delta wraps the same way.  lzf_host_parse_long is the
 * same rule on the host, with no HIP call: 1 and *out, or 0 (len == 0 and a
 * NULL pointer included).  One lane walks an entry's value serially: a
 * megabyte of digits costs one lane a megabyte of reads.
 *
 * A converted number gets a fresh 8-byte slot appended to the arena in list
 * order: for the k-th entry, val_off[i] = base + 8 * (CONVERTED entries
 * before k) with base = *store_used, val_size[i] = 8, enc[i] =
 * LZF_ENC_NUMBER, and *store_used = base + 8 * converted.  The old PLAIN
 * bytes become dead space, which lzf_gpu_store_compact reclaims.  Offsets are
 * dense and not 8-aligned: numbers are read and written at any alignment.
 *
 * *status (one device u32): LZF_STORE_OK, or LZF_STORE_FULL when base + 8 *
 * converted > store_cap or the sum wraps.  Then nothing changes -- not store,
 * val_off, val_size, enc, last_access, *store_used, entry_status or
 * entry_value -- and result is all zero.
 *
 * A NUMBER item whose val_size != 8 or whose [val_off, val_off + 8) leaves
 * [0, store_cap), and a PLAIN item whose [val_off, val_off + val_size) does,
 * is NAN and is not dereferenced.
 *
 * item_lock == NULL: nothing is locked; item_time and item_ttl: both NULL
 * (nothing expires) or both given; a non-NULL item_lock needs item_time.
 * result (6 device u64): [0] found = DONE + CONVERTED + UNCHANGED (the reply
 * of gbQueryMultiIncDecHandler), [1] expired, [2] locked, [3] nan,
 * [4] converted, [5] unchanged.  entry_value (n device i64, optional): the new
 * number for DONE and CONVERTED, the payload of the single-key REPL_VAL reply,
 * 0 otherwise.  work: lzf_gpu_store_minc_work_size(n) bytes of device scratch
 * that must stay valid until the stream's work is done.
 */
uint64_t lzf_gpu_store_minc_work_size(uint32_t n);
int lzf_gpu_store_minc(const uint32_t *idx, uint32_t n, int64_t delta, int single,
                       uint8_t *store, uint64_t store_cap, uint64_t *store_used,
                       uint64_t *val_off, uint32_t *val_size, uint8_t *enc, uint32_t count,
                       const int64_t *item_time, const int32_t *item_ttl,
                       const int64_t *item_lock /* may be NULL */, int64_t now,
                       int64_t *last_access /* may be NULL */,
                       uint8_t *entry_status /* may be NULL */, int64_t *entry_value /* may be NULL, n */,
                       uint64_t *result /* 6 u64 */, uint32_t *status, void *work, void *stream);
int lzf_host_parse_long(const uint8_t *v, uint32_t len, int64_t *out);

/*
 * SET on a locked key (src/query.c:446-451).  Runs between a
 * lzf_gpu_key_index_lookup of the new items' own keys -- occ[n], the lookup's
 * output for the items [first, first + n) -- and their
 * lzf_gpu_key_index_insert.  Per k, with j = occ[k]: if j < count, j lies
 * outside [first, first + n), enc[j] != LZF_ENC_NULL and item j is locked,
 * then enc[first + k] = LZF_ENC_NULL, refused[k] = 1 and result[0] grows by
 * one; otherwise refused[k] = 0.  The reference tests no validity here, so
 * neither does this.  The insert then skips the new item, its stored bytes are
 * dead space, and the old item stays the key's mapping.  refused (n device
 * bytes) may be NULL; result: 1 device u64.  LZF_GPU_EARG also for
 * first + n > count.  So set_store -> lookup -> set_guard -> insert queues on
 * one stream, and the host reads `refused` back with the reply.
 */
int lzf_gpu_store_set_guard(const uint32_t *occ, uint32_t first, uint32_t n, uint8_t *enc, uint32_t count,
                            const int64_t *item_time, const int64_t *item_lock, int64_t now,
                            uint8_t *refused /* may be NULL */, uint64_t *result /* 1 u64 */, void *stream);

/*
 * MSET by prefix: one new value for every entry of the list,
 * gbQueryMultiSetHandler / gbMultiSetCallback (src/query.c:479-537).
 *
 * Per entry, in this order (:490-502): dead -> DEAD; locked -> LOCKED,
 * untouched -- the lock is tested first, on an expired item too (:493 comes
 * before :496); expired -> EXPIRED, nulled; otherwise the item is replaced by
 * what gbSingleSet + gbCreateItem make (:375-425, :113-146) -> DONE: the new
 * stored bytes, val_size[i] and enc[i], val_len[i] = vlen, item_time[i] =
 * last_access[i] = now, item_ttl[i] = -1, and item_lock[i] = 0 when item_lock
 * is given.  The item keeps its index and its key, so a key index over the
 * store stays valid with no insert.
 *
 * The stored form is decided once, exactly as lzf_gpu_set_store decides it
 * for that one value, bit for bit: the value is compressed iff vlen >
 * compression, with out_len = vlen - 4 (for vlen < 4 the size wraps: no
 * limit); with a stream the stored form is LZF_ENC_LZF and S is the stream's
 * length, without one it is LZF_ENC_PLAIN, S = vlen and the input bytes.  The
 * reference compresses the same bytes once per matched key; this call does it
 * once.
 *
 * Placement: the k-th DONE entry in list order gets its own copy of the S
 * bytes at val_off[i] = base + S * (DONE entries before k), base =
 * *store_used, and *store_used = base + S * done.  The old bytes become dead
 * space, which lzf_gpu_store_compact reclaims.  *status (one device u32):
 * LZF_STORE_OK, or LZF_STORE_FULL when base + S * done > store_cap or the sum
 * wraps.  Then nothing at all changes -- no array, not *store_used, not
 * entry_status -- and result is all zero.
 *
 * result (5 device u64): [0] set (the reply of gbQueryMultiSetHandler; 0 ->
 * REPL_ERR_NOT_FOUND), [1] expired, [2] locked, [3] S, [4] the stored
 * encoding.  [3] and [4] are written on LZF_STORE_OK even when [0] is 0.  The
 * STATS fold, which the reference applies once per key set (:400-405): when
 * result[4] == LZF_ENC_LZF, lzf_host_store_stats over result[0] items that
 * all have enc = LZF_ENC_LZF, val_size = result[3] and val_len = vlen.
 *
 * `value` (vlen device bytes) must not overlap the arena's free part
 * [*store_used, store_cap): the copies are written there while the value is
 * read.  That cannot be checked.  item_time and item_ttl are required (they
 * are written); item_lock == NULL: nothing is locked.  LZF_GPU_EARG, before
 * any HIP call: a NULL required pointer, n == 0, count == 0, store_cap == 0,
 * vlen == 0 (the reference asserts vlen > 0), vlen > LZF_GPU_MAX_VALUE.
 * work: lzf_gpu_store_mset_work_size(n, vlen) bytes of device scratch that
 * must stay valid until the stream's work is done.  Asynchronous on `stream`,
 * with no host wait; the list rules of the operators above apply.
 */
uint64_t lzf_gpu_store_mset_work_size(uint32_t n, uint32_t vlen);
int lzf_gpu_store_mset(const uint32_t *idx, uint32_t n,
                       const uint8_t *value, uint32_t vlen, uint32_t compression,
                       uint8_t *store, uint64_t store_cap, uint64_t *store_used,
                       uint64_t *val_off, uint32_t *val_size, uint8_t *enc, uint32_t *val_len, uint32_t count,
                       int64_t *item_time, int32_t *item_ttl, int64_t *item_lock /* may be NULL */, int64_t now,
                       int64_t *last_access /* may be NULL */, uint8_t *entry_status /* may be NULL */,
                       uint64_t *result /* 5 u64 */, uint32_t *status, void *work, void *stream);

/*
 * The memory sweep, gbMemoryFreeHandler (src/server.c:311-327) over the whole
 * store: for a live item, eta = now - last_access[i] in two's complement, and
 * the item is freed (enc[i] = LZF_ENC_NULL) iff eta != 0 && eta >= gc_ratio,
 * compared signed.  Locks and TTLs are not consulted; the reference does not
 * consult them either.  result (3 device u64): [0] items freed, [1] the sum of
 * their val_size -- what a lzf_gpu_store_compact will reclaim -- [2] 1 if the
 * sweep ran.
 *
 * The gate is the cron's memused > maxmem (:401-411) without a host read:
 * with gate != NULL (one device u64, normally store_used) the sweep runs only
 * when *gate > max_bytes; otherwise nothing is written but result = {0, 0, 0}.
 * gate == NULL: the sweep runs.  LZF_GPU_EARG: a NULL last_access, enc,
 * val_size or result, count == 0.
 */
int lzf_gpu_store_gc(const int64_t *last_access, int64_t now, int64_t gc_ratio,
                     uint8_t *enc, const uint32_t *val_size, uint32_t count,
                     const uint64_t *gate /* may be NULL */, uint64_t max_bytes,
                     uint64_t *result /* 3 u64 */, void *stream);

/*
 * META, gbQueryMetaHandler / gbGetItemMeta (src/query.c:1255-1339), over an
 * index list.
 *
 * lzf_host_meta_field (host, no HIP call) resolves the field name exactly as
 * gbGetItemMeta's chain does, quirks included: strncmp(m, name, min(mlen,
 * strlen(name))) == 0, tried in the order size, encoding, access, created,
 * ttl, left, lock.  So "s" and "sizeXYZ" are size, and "l" is left, not lock;
 * a NUL inside m ends the comparison as strncmp does.  Returns the LZF_META_*
 * code, or -1 (mlen == 0 and a NULL pointer included).  For an unknown field
 * the reference still updates last_access on a valid item and replies
 * REPL_ERR: that path is the host's reply plus lzf_gpu_store_count over the
 * entry.
 *
 * lzf_gpu_store_meta, per entry: dead -> DEAD; expired -> EXPIRED and nulled
 * (gbIsNodeStillValid, remove = 1); valid -> entry_value[k] is written, then
 * last_access[i] = now -> DONE, so ACCESS reports the value before this call
 * (:1322-1330).  Locks are not tested.  The values: SIZE val_size[i] (the
 * stored size, as the reference), ENCODING enc[i], ACCESS last_access[i],
 * CREATED item_time[i], TTL item_ttl[i], LEFT ttl <= 0 ? -1 : ttl - (now -
 * item_time[i]), LOCK item_lock[i], or 0 when item_lock is NULL.
 * entry_value[k] (n device i64, required) is 0 for entries that are not DONE.
 * item_time and item_ttl are required; last_access may be NULL, but not for
 * ACCESS.  result (2 device u64): [0] found, [1] expired.  LZF_GPU_EARG also
 * for a field outside 0..6, n == 0, count == 0.
 */
#define LZF_META_SIZE      0
#define LZF_META_ENCODING  1
#define LZF_META_ACCESS    2
#define LZF_META_CREATED   3
#define LZF_META_TTL       4
#define LZF_META_LEFT      5
#define LZF_META_LOCK      6
int lzf_host_meta_field(const uint8_t *m, uint32_t mlen);   /* code, or -1 */
int lzf_gpu_store_meta(const uint32_t *idx, uint32_t n, int field, uint8_t *enc, const uint32_t *val_size,
                       uint32_t count, const int64_t *item_time, const int32_t *item_ttl,
                       const int64_t *item_lock /* may be NULL: 0 */, int64_t now,
                       int64_t *last_access /* may be NULL, but not for ACCESS */,
                       uint8_t *entry_status /* may be NULL */, int64_t *entry_value,
                       uint64_t *result /* 2 u64: found, expired */, void *stream);

/*
 * The KEYS reply, gbQueryKeysHandler (src/query.c:1341-1391) after tr_search,
 * over an index list (a lzf_gpu_store_select_prefix's output).
 *
 * An entry takes part iff it is in range, enc[i] != LZF_ENC_NULL and
 * key_len[i] > 0.  The reference makes no validity test here: an expired item
 * that has not been nulled takes part, nothing is nulled and last_access is
 * not written.  The j-th participating entry in list order becomes the pair
 *   [u32 ndigits][digits][u8 LZF_ENC_PLAIN][u32 key_len][key bytes]
 * whose KVAL key is the decimal text of j ("%lu": "0", no leading zeros) and
 * whose value is the item's key as a PLAIN item.  The pairs are preceded by
 * [u32 found] and, with reply_header, by the 7-byte header -- byte for byte
 * what lzf_gpu_kv_frame writes for the same pairs.
 *
 * result (2 device u64): [0] found, [1] LZF_MGET_OK, LZF_MGET_NOT_FOUND
 * (found == 0) or LZF_MGET_TOO_BIG (the payload, header excluded, >
 * max_response).  In the two last cases *frame_len = 0 and no frame byte is
 * written; otherwise *frame_len is the frame's size, header included.  No byte
 * at or past (reply_header ? 7 : 0) + max_response is ever written.
 *
 * Keys containing a NUL byte are outside the model: the reference truncates
 * them through strlen (:1367), this call writes all key_len bytes.  Reply
 * order is list order (lzf_gpu_store_select_ordered gives the reference's).  work:
 * lzf_gpu_store_keys_work_size(n) bytes of device scratch that must stay valid
 * until the stream's work is done.  LZF_GPU_EARG: a NULL pointer, n == 0,
 * count == 0.
 */
uint64_t lzf_gpu_store_keys_work_size(uint32_t n);
int lzf_gpu_store_keys(const uint32_t *idx, uint32_t n,
                       const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len,
                       const uint8_t *enc, uint32_t count, int reply_header,
                       uint8_t *frame, uint64_t max_response, uint64_t *frame_len,
                       uint64_t *result /* 2 u64: found, LZF_MGET_* */, void *work, void *stream);

/*
 * The device key index: exact-key lookup and upsert for the device store.
 *
 * The operators above address items by index.  The key index maps key bytes
 * to an item index in device memory, so that a request buffer of keys goes in
 * and an index list comes out with no host lookup: insert is tr_insert plus
 * gbDestroyItem(old) (src/query.c:418-422) for the items a lzf_gpu_set_store
 * has just written, lookup is tr_find_node for a batch of query keys.
 *
 * The table is caller-owned device memory of lzf_gpu_key_index_bytes(slots)
 * bytes, 8-byte aligned; slots is a power of two in [16, 2^31] (otherwise the
 * size is 0 and every call LZF_GPU_EARG).  Its layout is opaque but for two
 * fixed points: a table filled with byte 0xFF is empty, so
 * hipMemsetAsync(table, 0xFF, bytes) clears it, and the probe sequence of a
 * key is home, home + 1, ... modulo slots (linear probing), home being
 * lzf_host_key_home(key, len, slots).  `used` is one device u32 that the
 * caller owns and zeroes together with the table; it counts claimed slots.
 *
 * A slot names an item index of the store.  Key bytes are never copied into
 * the table: they are read from keys / key_off / key_len (as lzf_gpu_kv_frame
 * takes them), which must therefore stay intact for dead items too until the
 * table is rebuilt.  A slot never returns to empty except by a clear, so
 * chains never break: the slot of an item that has gone dead (enc[i] ==
 * LZF_ENC_NULL) keeps its place and a later insert of the same key takes it
 * over.
 *
 * Rebuild: clear the table and *used, then insert [0, count) --
 * lzf_gpu_key_index_rebuild does all of it on the stream.  Dead items drop out
 * and *used becomes the number of distinct live keys.  It belongs with
 * lzf_gpu_store_compact and lzf_gpu_store_renumber, the store's housekeeping,
 * run when lzf_gpu_store_usage shows enough dead items.  Item indices survive
 * a compaction and a rebuild; after a renumbering the table names old indices
 * and must be rebuilt over the new arrays before the next lookup.
 *
 * Locks: SET on a locked item replies REPL_ERR_LOCKED (src/query.c:446-451);
 * lzf_gpu_store_set_guard, run between the lookup of a batch's own keys and
 * its insert, decides that on the device.  Not modelled: the SET reply, which
 * the host builds from the request's bytes it holds.  (The ordered prefix walk
 * is lzf_gpu_store_select_ordered.)
 */
#define LZF_KIDX_OK    0
#define LZF_KIDX_FULL  1   /* *used + n > slots - slots / 4: the batch was refused as a whole */

uint64_t lzf_gpu_key_index_bytes(uint32_t slots);
/* host, no HIP call: the home slot the device uses for a key; 0xFFFFFFFF for a
 * bad `slots`.  For sizing, and for building a chain on purpose. */
uint32_t lzf_host_key_home(const uint8_t *key, uint32_t len, uint32_t slots);

/*
 * Upsert of the items [first, first + n) of a store of `count` items.  The
 * outcome is that of the loop, in ascending i over the batch:
 *   skip i if enc[i] == LZF_ENC_NULL or key_len[i] == 0 (the reference
 *   asserts klen > 0); j = map.get(key_i); if j exists, j != i and j is live:
 *   enc[j] = LZF_ENC_NULL; map[key_i] = i
 * whatever order the device's threads run in:
 *   - among batch items with equal keys the highest index ends as the key's
 *     mapping, the others get enc = LZF_ENC_NULL ("superseded");
 *   - a batch item always beats an occupant from outside the batch, whatever
 *     the two indices are (callers may reuse low indices): a live occupant
 *     gets enc = LZF_ENC_NULL ("replaced"), the slot of a dead one is simply
 *     taken over, and *used grows in neither case;
 *   - an occupant that lies in the batch takes part as the batch item it is,
 *     so inserting a range that is already indexed changes nothing.
 * result (4 device u64): [0] batch items that are their key's mapping after
 * the call, [1] replaced, [2] superseded, [3] skipped.  *used grows by the
 * number of slots newly claimed.
 *
 * *status (one device u32): LZF_KIDX_OK, or LZF_KIDX_FULL exactly when
 * *used + n > slots - slots / 4 (n counted whole, skipped items included),
 * judged on *used as it was before the call.  Then the batch is refused as a
 * whole: no table byte, no enc and not *used change, and result is zero.  The
 * host reads status back with the reply; the remedy is a larger table and a
 * rebuild.  Until then the batch's items are live in the store but NOT
 * findable by key -- a lookup misses them and a later SET of the same key
 * does not replace them.
 *
 * LZF_GPU_EARG, before any HIP call: a NULL pointer, count == 0, n == 0,
 * first + n > count (64-bit arithmetic), a bad `slots`, a table that is not
 * 8-byte aligned.  Asynchronous on `stream`, with no host wait.
 */
int lzf_gpu_key_index_insert(void *table, uint32_t slots, uint32_t *used,
                             const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len,
                             uint8_t *enc, uint32_t count, uint32_t first, uint32_t n,
                             uint64_t *result /* 4 u64 */, uint32_t *status, void *stream);

/*
 * Rebuild: the table and *used are cleared on the stream, then every item of
 * [0, count) is inserted, as lzf_gpu_key_index_insert(first = 0, n = count)
 * into an empty table does -- with one difference.  LZF_KIDX_FULL is judged on
 * the number of items the insert will not skip (live and key_len > 0), counted
 * on the device, not on count: it is FULL exactly when that number exceeds
 * slots - slots / 4.  So count = dst_cap after a lzf_gpu_store_renumber whose
 * `live` the host has not read yet is not refused for its dead tail.  On FULL
 * the table stays cleared, *used is 0, result is zero and no enc changes.
 * Otherwise result and the superseding of duplicate live keys are the
 * insert's: the highest index wins, which after a renumbering (stable) is the
 * winner from before it.  result[0] serves as the counting word before the
 * decision; there is no work area.  LZF_GPU_EARG, before any HIP call: a NULL
 * pointer, count == 0, a bad `slots`, a table that is not 8-byte aligned.
 * Asynchronous on `stream`, with no host wait.
 */
int lzf_gpu_key_index_rebuild(void *table, uint32_t slots, uint32_t *used,
                              const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len,
                              uint8_t *enc, uint32_t count,
                              uint64_t *result /* 4 u64 */, uint32_t *status, void *stream);

/*
 * Lookup of nq query keys (qkeys / q_off / q_len, an arena of their own or
 * the store's).  idx[k] is the item index the key maps to, or 0xFFFFFFFF when
 * the key is absent, its item is dead, or q_len[k] == 0.  An expired item is a
 * hit, as tr_find_node returns it: the consuming operator applies the TTL
 * rule and nulls it, exactly as after a prefix select.  0xFFFFFFFF is the
 * padding every index-list operator ignores, so idx feeds them unchanged:
 * lzf_gpu_store_mget is the frame for many exact keys in query order,
 * lzf_gpu_store_count followed by lzf_gpu_store_delete is DEL by key,
 * lzf_gpu_store_mttl sets TTLs by key.
 *
 * result (3 device u64): [0] hits, [1] misses, [2] slots examined, summed over
 * the queries (the empty slot that ends a miss counts).  A lookup examines at
 * most `slots` slots per key, so it terminates on any table contents; a slot
 * naming an index >= count is a non-matching occupant and is never
 * dereferenced.  LZF_GPU_EARG: a NULL pointer, count == 0, nq == 0, a bad
 * `slots`, a table that is not 8-byte aligned.
 */
int lzf_gpu_key_index_lookup(const void *table, uint32_t slots,
                             const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len,
                             const uint8_t *enc, uint32_t count,
                             const uint8_t *qkeys, const uint64_t *q_off, const uint32_t *q_len, uint32_t nq,
                             uint32_t *idx, uint64_t *result /* 3 u64 */, void *stream);

/*
 * Per-request replies over an index list: the reply of GET, and of the
 * single-key INC / DEC, for the requests of many clients batched into one
 * list (lzf_gpu_key_index_lookup yields it).  For n entries the call writes n
 * self-contained reply frames into one reply arena in device memory, LZF
 * items decoded in place, asynchronously on `stream` with no host wait:
 * lookup -> replies -> one copy of replies[0 .. *rep_used), rep_off, rep_len.
 *
 * A reply is the buffer of gbClientEnqueueData (src/net.c:1170-1202):
 *   [i16 code LE][u8 encoding][u32 size LE][size bytes]
 * A code reply is gbClientEnqueueCode's form of it: encoding PLAIN, size 1,
 * one 0x00 byte -- 8 bytes.  An item reply is gbClientEnqueueItem's
 * (src/net.c:1216-1254), code REPL_VAL, by the item's encoding:
 *   PLAIN   the val_size stored bytes;
 *   NUMBER  the stored bytes, encoding NUMBER;
 *   LZF     encoding PLAIN, size val_len, the value decoded straight into the
 *           reply.
 * The framing is a restatement of src/net.c, not compared with a build of it.
 *
 * mode LZF_REPLY_GET, gbQueryGetHandler (src/query.c:634-663): the validity
 * rule as MGET applies it.  A dead, out-of-range or padding entry is
 * LZF_ENT_DEAD and gets a REPL_ERR_NOT_FOUND code reply; an expired entry is
 * LZF_ENT_EXPIRED, is nulled in enc and gets the same reply; a valid entry is
 * LZF_ENT_DONE, gets last_access[i] = now and its item reply.  Every copy of a
 * duplicated entry is judged on what enc held before the call and gets a
 * reply of its own: two clients asking for one key are the normal case.
 * op_status must be NULL.
 *
 * mode LZF_REPLY_VALUE, the reply after an operator that left entry_status
 * (lzf_gpu_store_minc(single = 1)): no validity rule is applied and neither
 * enc nor last_access is written.  op_status[k] (n device bytes, required) is
 * mapped by the rule of lzf_host_reply_code: DONE and CONVERTED -> REPL_VAL,
 * an item reply of item idx[k] as it now stands; DEAD and EXPIRED ->
 * REPL_ERR_NOT_FOUND; LOCKED -> REPL_ERR_LOCKED; NAN and UNCHANGED ->
 * REPL_ERR_NAN; anything else -> REPL_ERR.  An entry mapped to REPL_VAL whose
 * idx[k] >= count or whose enc[idx[k]] is LZF_ENC_NULL gets REPL_ERR.
 * entry_status[k] = op_status[k] (but for decode failures, below); the two
 * may be the same array.
 *
 * The arena.  Replies are packed densely in list order from byte 0.  The slot
 * of a reply is max(8, 7 + size) bytes -- a size-0 PLAIN item writes 7 bytes
 * into an 8-byte slot -- rep_off[k] is the exclusive sum of the slots,
 * rep_len[k] the reply's byte count and *rep_used the sum of the slots.  No
 * byte at or past rep_cap is ever written.  If the slots do not fit in
 * rep_cap the call is LZF_REPLY_TOO_BIG: no arena byte is written and
 * *rep_used = 0, while rep_off, rep_len and entry_status are written as they
 * would have been and result[4] holds the bytes needed, so the host retries
 * with a larger arena.  GET's nulling and last_access happen whatever the
 * status, as in MGET.
 *
 * Decode failures are per entry.  An LZF item fails when it does not decode
 * to exactly val_len bytes: a decoder error, a wrong length, or val_len >
 * max_val_len (above LZF_GPU_MAX_VALUE: LZF_GPU_EARG).  The entry is
 * LZF_ENT_EDECODE, a REPL_ERR code reply stands at the start of its slot,
 * rep_len[k] = 8, the rest of its slot is unspecified and nothing outside it
 * is touched; the other replies are unaffected.  An item refused for val_len >
 * max_val_len is known before the layout is made and takes an 8-byte slot.
 * The decoder runs once over the list, bounded by max_val_len, as MGET's does.
 * LZF_GPU_REPLY_ONE_ROUTE=0 (diagnostics) runs it once per decode size class
 * (lzf_gpu_size_class) instead, each launch over its own entries with its
 * class's bound and still with no host wait; that form measured slower on a
 * list of mixed sizes, so it is not the default.
 *
 * result (6 device u64): [0] item replies, [1] entries this call expired,
 * [2] dead or skipped entries -- in VALUE mode: the code replies -- [3] one of
 * LZF_REPLY_*, [4] the bytes needed, [5] decode failures.  [0] + [1] + [2] +
 * [5] == n.  On LZF_REPLY_TOO_BIG nothing is decoded: [5] counts the refused
 * items only.
 *
 * LZF_GPU_EARG, before any HIP call: a NULL pointer but the optional ones,
 * n == 0, count == 0, a bad mode, op_status not matching the mode, exactly
 * one of item_time / item_ttl NULL, max_val_len > LZF_GPU_MAX_VALUE.  work:
 * lzf_gpu_store_replies_work_size(n) bytes of device scratch that must stay
 * valid until the stream's work is done.  The SET reply stays with the host.
 */
#define LZF_REPL_ERR            0   /* src/query.h:64-70 */
#define LZF_REPL_ERR_NOT_FOUND  1
#define LZF_REPL_ERR_NAN        2
#define LZF_REPL_ERR_LOCKED     4
#define LZF_REPL_OK             5
#define LZF_REPL_VAL            6
#define LZF_ENT_EDECODE         7   /* replies: an LZF item did not decode to val_len */

#define LZF_REPLY_GET    0   /* gbQueryGetHandler, src/query.c:634-663 */
#define LZF_REPLY_VALUE  1   /* after an operator that left entry_status (single-key INC / DEC) */

#define LZF_REPLY_OK       0
#define LZF_REPLY_TOO_BIG  1   /* the slots do not fit in rep_cap */

uint64_t lzf_gpu_store_replies_work_size(uint32_t n);
int lzf_gpu_store_replies(const uint32_t *idx, uint32_t n, int mode,
                          const uint8_t *op_status /* VALUE: n LZF_ENT_* bytes, required; GET: must be NULL */,
                          const uint8_t *store, const uint64_t *val_off, const uint32_t *val_size,
                          uint8_t *enc, const uint32_t *val_len, uint32_t count,
                          const int64_t *item_time, const int32_t *item_ttl, int64_t now,
                          int64_t *last_access /* may be NULL */, uint32_t max_val_len,
                          uint8_t *replies, uint64_t rep_cap, uint64_t *rep_used,
                          uint64_t *rep_off /* n */, uint32_t *rep_len /* n */, uint8_t *entry_status /* n */,
                          uint64_t *result /* 6 u64 */, void *work, void *stream);
/* host, no HIP call: the LZF_REPL_* code of an LZF_ENT_* entry status */
int lzf_host_reply_code(int ent_status);

/*
 * Request ingest: raw request buffers in, the descriptors of every call above
 * out, without the host reading a request.
 *
 * A request is what gbProcessQuery sees (src/query.c:1393-1485): client->buffer
 * of buffer_size bytes, [i16 opcode, little-endian][payload], size =
 * buffer_size - 2; the wire's 4-byte length prefix is not part of it.  Request
 * k of a batch is req[req_off[k] .. + req_len[k]) in one arena of req_bytes
 * bytes.  The parse is the reference's, quirk for quirk (src/query.c:229-373):
 *
 *   grammar                       operators                         num
 *   key only                      GET DEL INC DEC UNLOCK MDEL MINC  -
 *                                 MDEC MUNLOCK COUNT KEYS
 *   key and required value        MSET (the value), META (a field)  -
 *   key and required number       TTL MTTL LOCK MLOCK               lzf_host_parse_long of the value
 *   key and optional number       MGET                              the limit, -1 without a value
 *   ttl, key, value               SET                               the raw ttl (:444)
 *   no payload read               STATS PING END                    -
 *
 * The key scan stops at the first ' ' or after end = min(size, max_key) bytes;
 * SET's ttl token and key share one budget of end (:334-347); one byte is
 * skipped after each token, space or not; the value is size - ttllen - klen -
 * 2 bytes (SET), size - klen - 1 (key and value) or left - 1 (MGET), clamped
 * to max_value; the checks run in the order ttl token, key, value.
 *
 * status[k] is one of LZF_REQ_*.  LZF_REQ_SHORT is the one deliberate
 * departure from the reference: where the payload ends with the key ("10 key"
 * for SET, "abc" for TTL, a key of exactly max_key bytes with nothing behind
 * it) the reference's unsigned subtraction wraps, min() makes it maxvaluesize
 * and the handler reads past its buffer; here the request is refused and the
 * reply is REPL_ERR.  Every status but OK and NAN leaves the spans and num 0;
 * NAN keeps its spans, because the single-key TTL and LOCK handlers look the
 * key up before they test the number (:553-565, :983-985): the caller needs
 * the key to choose between REPL_ERR_NOT_FOUND and REPL_ERR_NAN.
 *
 * Outputs, n entries each: op (u8: 1-21, 0xFF, or 0 for BADOP and ERANGE),
 * status (u8), key_off (u64) / key_len (u32), val_off (u64) / val_len (u32),
 * num (i64).  The offsets are absolute into req (0 with a length of 0), so the
 * outputs feed the calls above as they are: for lzf_gpu_set_store req is `in`,
 * val_off is in_off and lzf_gpu_store_append_keys' set_len is in_len; for
 * lzf_gpu_key_index_lookup req is qkeys and key_off / key_len are q_off /
 * q_len.  A key_len of 0 is a miss in the lookup, so a refused request is
 * padding for every index-list operator.  With expect_op != 0 a request with
 * any other (known) opcode gets LZF_REQ_OTHER and zero spans.  result
 * (LZF_REQ_NSTATUS device u64): how many requests got each status.
 *
 * No byte outside [req, req + req_bytes) is read and no output depends on a
 * byte outside the request's own range.  LZF_GPU_EARG, before any HIP call: a
 * NULL pointer, n == 0, max_key == 0, max_value == 0.  Asynchronous on
 * `stream`, with no host wait.  lzf_host_request_parse is the same function in
 * a host loop over host arrays, with no HIP call.
 */
#define LZF_OP_SET      1    /* src/query.h:37-59 */
#define LZF_OP_TTL      2
#define LZF_OP_GET      3
#define LZF_OP_DEL      4
#define LZF_OP_INC      5
#define LZF_OP_DEC      6
#define LZF_OP_LOCK     7
#define LZF_OP_UNLOCK   8
#define LZF_OP_MSET     9
#define LZF_OP_MTTL     10
#define LZF_OP_MGET     11
#define LZF_OP_MDEL     12
#define LZF_OP_MINC     13
#define LZF_OP_MDEC     14
#define LZF_OP_MLOCK    15
#define LZF_OP_MUNLOCK  16
#define LZF_OP_COUNT    17
#define LZF_OP_STATS    18
#define LZF_OP_PING     19
#define LZF_OP_META     20
#define LZF_OP_KEYS     21
#define LZF_OP_END      0xFF

#define LZF_REQ_OK       0   /* parsed */
#define LZF_REQ_ERR      1   /* the parse function returns 0 (REPL_ERR); SET with size 0 */
#define LZF_REQ_NAN      2   /* the number does not parse (REPL_ERR_NAN); the spans are kept */
#define LZF_REQ_BADOP    3   /* no branch in gbProcessQuery, or shorter than 2 bytes: GB_ERR, drop the client */
#define LZF_REQ_SHORT    4   /* the value span would leave the request (the reference over-reads) */
#define LZF_REQ_ERANGE   5   /* req_off + req_len > req_bytes */
#define LZF_REQ_OTHER    6   /* a known opcode, but not expect_op */
#define LZF_REQ_NSTATUS  7

int lzf_gpu_request_parse(const uint8_t *req, uint64_t req_bytes,
                          const uint64_t *req_off, const uint32_t *req_len, uint32_t n,
                          uint32_t max_key, uint32_t max_value, uint32_t expect_op,
                          uint8_t *op, uint8_t *status, uint64_t *key_off, uint32_t *key_len,
                          uint64_t *val_off, uint32_t *val_len, int64_t *num,
                          uint64_t *result /* LZF_REQ_NSTATUS u64 */, void *stream);
int lzf_host_request_parse(const uint8_t *req, uint64_t req_bytes,
                           const uint64_t *req_off, const uint32_t *req_len, uint32_t n,
                           uint32_t max_key, uint32_t max_value, uint32_t expect_op,
                           uint8_t *op, uint8_t *status, uint64_t *key_off, uint32_t *key_len,
                           uint64_t *val_off, uint32_t *val_len, int64_t *num,
                           uint64_t *result /* LZF_REQ_NSTATUS u64 */);
/* host, no HIP call: -1 for LZF_REQ_OK (the operator replies), -2 for
 * LZF_REQ_BADOP (close the connection), LZF_REPL_ERR_NAN for LZF_REQ_NAN,
 * LZF_REPL_ERR otherwise */
int lzf_host_request_reply_code(int status);

/*
 * SET's other half: the keys of a parsed SET batch appended to the store's key
 * arena and the new items' key and time members filled, so that
 * lzf_gpu_set_store can follow without the host knowing a key.
 *
 * The call serves the n requests of a batch as lzf_gpu_request_parse left
 * them (op, status, rq_key_off, rq_key_len, rq_val_len, num; req / req_bytes
 * the same arena).  Item first + k belongs to request k, accepted or not, so
 * the caller needs no count from the device.  Request k is accepted iff
 * op[k] == LZF_OP_SET, status[k] == LZF_REQ_OK and [rq_key_off[k], +
 * rq_key_len[k]) lies inside [0, req_bytes) (64-bit, wrap-safe); otherwise it
 * is refused.
 *
 * Accepted: the key bytes are appended to `keys`, dense and in request order,
 * from base = *keys_used; key_off[first + k] = base + the accepted key bytes
 * before k, key_len[first + k] = rq_key_len[k]; item_time = last_access = now,
 * item_lock = 0, item_ttl = num > 0 ? min(max_item_ttl, num) : -1
 * (gbCreateItem at src/query.c:113-128, then :454-458); set_len[k] =
 * rq_val_len[k]; void_idx[k] = 0xFFFFFFFF.
 * Refused: key_len = 0 and key_off the running end offset (the tie that
 * renumbering's tail leaves); the time members as for a fresh item without a
 * TTL (item_ttl -1); set_len[k] = 0; void_idx[k] = first + k.  After
 * lzf_gpu_set_store(in = req, in_off = val_off, in_len = set_len) has run,
 * lzf_gpu_store_delete(void_idx, n, ...) nulls the refused requests' items: a
 * refused request costs zero bytes and one burnt index.
 *
 * result (4 device u64): [0] accepted, [1] refused, [2] key bytes appended,
 * [3] LZF_STORE_OK or LZF_STORE_FULL.  FULL -- base + the accepted key bytes
 * exceed keys_cap or wrap -- is decided before any byte is written and refuses
 * the call whole: no byte of `keys` is written, *keys_used is unchanged, every
 * request is refused as above (set_len 0, void_idx first + k, key_len 0), and
 * result is [0, n, 0, LZF_STORE_FULL].  On OK *keys_used = base + result[2].
 *
 * item_time and item_ttl: both or neither; item_lock and last_access may be
 * NULL.  LZF_GPU_EARG, before any HIP call: a NULL pointer but those, n == 0,
 * count == 0, keys_cap == 0, first + n > count (64-bit), exactly one of
 * item_time / item_ttl.  `work`: lzf_gpu_store_append_keys_work_size(n) bytes
 * of device scratch that must stay valid until the stream's work is done.
 * Asynchronous on `stream`, with no host wait.
 *
 * One SET batch on one stream: lzf_gpu_request_parse ->
 * lzf_gpu_store_append_keys -> lzf_gpu_set_store -> lzf_gpu_store_delete(
 * void_idx) -> lzf_gpu_key_index_lookup of the new items' own keys ->
 * lzf_gpu_store_set_guard -> lzf_gpu_store_replies(LZF_REPLY_GET) over first
 * .. first + n (the SET reply, gbClientEnqueueItem(REPL_VAL, item) at :460;
 * before the insert, so that a batch's superseded duplicates still get their
 * own value back) -> lzf_gpu_key_index_insert.  The host overrides the reply
 * of a refused request from `status` and of a locked key from `refused`.
 *
 * Limits: a short key (below 256 bytes) is staged by one lane.
 */
uint64_t lzf_gpu_store_append_keys_work_size(uint32_t n);
int lzf_gpu_store_append_keys(const uint8_t *req, uint64_t req_bytes,
                              const uint8_t *op, const uint8_t *status,
                              const uint64_t *rq_key_off, const uint32_t *rq_key_len,
                              const uint32_t *rq_val_len, const int64_t *num, uint32_t n,
                              uint8_t *keys, uint64_t keys_cap, uint64_t *keys_used,
                              uint64_t *key_off, uint32_t *key_len,
                              int64_t *item_time, int32_t *item_ttl,
                              int64_t *item_lock /* may be NULL */, int64_t *last_access /* may be NULL */,
                              uint32_t first, uint32_t count, int64_t now, int32_t max_item_ttl,
                              uint32_t *set_len /* n */, uint32_t *void_idx /* n */,
                              uint64_t *result /* 4 u64 */, void *work, void *stream);

/*
 * Request dispatch: a parsed batch of mixed operators bucketed by operator on
 * the device, and the per-operator replies stitched back into request order,
 * so that one event-loop tick goes sockets -> one arena -> parse (expect_op =
 * 0) -> bucket -> per-operator calls -> stitch -> one copy, with the host
 * reading no request and overriding no reply.
 *
 * The class rule, lzf_host_request_class(op, status), LZF_RQ_NCLASS = 23
 * classes:
 *   0        refused: every status but LZF_REQ_OK and LZF_REQ_NAN (and an op
 *            the parse cannot yield: 0, 22 .. 254);
 *   1 .. 21  the operator itself, for status OK or NAN -- NAN keeps its spans
 *            and travels with its operator, because the TTL and LOCK handlers
 *            look the key up before they test the number;
 *   22       LZF_OP_END.
 *
 * lzf_gpu_request_bucket takes the seven outputs of a parse of n requests and
 * writes, all in device memory:
 *   perm[n]         request indices, class-major; inside a class the request
 *                   order is kept (a stable partition);
 *   slot[n]         the inverse, perm[slot[k]] == k;
 *   class_first[LZF_RQ_NCLASS + 1]
 *                   class c is perm[class_first[c] .. class_first[c + 1]),
 *                   class_first[LZF_RQ_NCLASS] == n;
 *   b_op .. b_num   the seven arrays in bucket order, b_x[j] = x[perm[j]].
 * Class c's slice is pointer + class_first[c] with class_first[c + 1] -
 * class_first[c] entries and feeds the calls above as it is, the offsets still
 * absolute into the request arena: b_key_off / b_key_len are
 * lzf_gpu_key_index_lookup's q_off / q_len; the SET slice has op == SET
 * throughout and status OK but for its NAN requests, which
 * lzf_gpu_store_append_keys refuses one by one, and b_val_off is
 * lzf_gpu_set_store's in_off.
 *
 * Asynchronous on `stream`, with no host wait inside the call.  The caller
 * copies the 96 bytes of class_first to size its per-class launches: one small
 * wait per batch, as lzf_gpu_*_mixed takes for its 48 bytes.  n up to 2^32 - 1,
 * 64-bit byte arithmetic.  LZF_GPU_EARG, before any HIP call: a NULL pointer,
 * n == 0.  `work`: lzf_gpu_request_bucket_work_size(n) bytes of device scratch
 * that must stay valid until the stream's work is done.
 * lzf_host_request_bucket is the same partition as a counting sort over host
 * arrays, with no HIP call.
 *
 * lzf_gpu_request_stitch builds the reply table in request order and makes
 * the overrides on the device.  It copies no reply byte: a client's reply
 * stays a slice of the one device-to-host copy of replies[0 .. rep_cap).
 * Inputs: op, status, slot (request order, n entries) and class_first (device);
 * class_mode and class_base, two HOST arrays of LZF_RQ_NCLASS entries that
 * travel in the kernel's arguments -- class_mode[c] is LZF_STITCH_HOST (the
 * host builds the class's replies: PING, STATS, END, and MGET / KEYS, whose
 * frames the host has from lzf_gpu_store_select_ordered and the operator),
 * LZF_STITCH_ARENA (lzf_gpu_store_replies wrote them) or LZF_STITCH_CODE (the
 * class left an entry status), class_base[c] is where class c's reply arena
 * starts inside `replies`; and in bucket order, n entries each, b_rep_off /
 * b_rep_len (what lzf_gpu_store_replies wrote for each ARENA class, at the
 * class's slice), b_ent (LZF_ENT_*: what lzf_gpu_store_mdel / _mlock /
 * _munlock left for each CODE class; may be NULL when no class is CODE) and
 * b_refused (lzf_gpu_store_set_guard's output at the SET slice; may be NULL).
 * code_base: 64 bytes of `replies` where the call writes the code frames of
 * the codes 0 .. 6, 8 bytes each, [i16 code][u8 PLAIN][u32 1][0x00]
 * (gbClientEnqueueCode's form); the frame of code c is at code_base + 8 c and
 * the last 8 bytes are zero.
 *
 * Request k, with j = slot[k] and c its class; the first rule that matches:
 *   1. status BADOP                    LZF_OUT_CLOSE, offset and length 0
 *   2. a status other than OK / NAN    the REPL_ERR frame
 *   3. NAN                             REPL_ERR_NOT_FOUND if c is CODE and
 *                                      b_ent[j] is DEAD or EXPIRED, otherwise
 *                                      REPL_ERR_NAN
 *   4. class_mode[c] == HOST           LZF_OUT_HOST, offset and length 0
 *   5. op SET, b_refused given and b_refused[j] != 0
 *                                      REPL_ERR_LOCKED
 *   6. ARENA                           out_off = class_base[c] + b_rep_off[j],
 *                                      out_len = b_rep_len[j]; a slice that
 *                                      leaves [0, rep_cap) or wraps (64-bit)
 *                                      becomes the REPL_ERR frame and counts
 *                                      in result[4]
 *   7. CODE                            DONE / CONVERTED -> REPL_OK, anything
 *                                      else lzf_host_reply_code(b_ent[j])
 * A table that contradicts itself -- status OK or NAN and slot[k] outside its
 * class's range of class_first, or >= n -- is treated as a bad slice after rule
 * 2 (REPL_ERR, counted in result[4]); no b_* entry is read for it.
 *
 * Outputs, request order: out_off (u64, absolute into replies), out_len (u32),
 * out_kind (u8, LZF_OUT_*).  result (5 device u64): [0] arena replies, [1]
 * code replies, [2] closes, [3] host, [4] bad slices (they are among [1]);
 * [0] + [1] + [2] + [3] == n.  Nothing is written outside the three output
 * arrays, result and the 64 code bytes.  LZF_GPU_EARG, before any HIP call: a
 * NULL required pointer, n == 0, a mode above 2, an ARENA class with b_rep_off
 * or b_rep_len NULL, a CODE class with b_ent NULL, code_base + 64 > rep_cap
 * (64-bit, wrap-safe).  Asynchronous on `stream`, with no host wait.
 * lzf_host_request_stitch is the same function in a host loop over host
 * arrays, with no HIP call.
 *
 * A mixed batch on one stream: lzf_gpu_request_parse(expect_op = 0) ->
 * lzf_gpu_request_bucket -> copy class_first -> per class, in an order the
 * caller chooses, the calls above over the class's slices (SET: the eight
 * steps of lzf_gpu_store_append_keys' contract; GET: lookup ->
 * lzf_gpu_store_replies; DEL / LOCK / UNLOCK: lookup -> lzf_gpu_store_mdel /
 * _mlock / _munlock with entry_status), each ARENA class into its own range
 * of `replies` -> lzf_gpu_request_stitch -> one copy of replies and the table.
 *
 * The batch's serial order.  A bucketed batch executes class by class in the
 * order the caller launches the classes, and inside a class in request order:
 * that is one serial order of the batch.  It is a legal outcome of the
 * reference server exactly when no client has two requests in the batch --
 * requests of different clients in one tick have no order a client can
 * observe -- so a client's next request waits for the next batch.  Limits:
 * the index-list operators leave duplicates unspecified, so two DELs or INCs
 * of one key in one batch are the host's to split; the prefix operators'
 * reply order (MGET with a limit, KEYS) comes from
 * lzf_gpu_store_select_ordered, which the host queues in front of them.
 */
#define LZF_RQ_NCLASS      23

#define LZF_STITCH_HOST    0
#define LZF_STITCH_ARENA   1
#define LZF_STITCH_CODE    2

#define LZF_OUT_REPLY      0   /* out_len bytes at replies + out_off */
#define LZF_OUT_CLOSE      1   /* close the connection (gbProcessQuery returns GB_ERR) */
#define LZF_OUT_HOST       2   /* the host builds this reply */

/* host, no HIP call: the class of (op, status), 0 .. LZF_RQ_NCLASS - 1 */
int lzf_host_request_class(int op, int status);
uint64_t lzf_gpu_request_bucket_work_size(uint32_t n);
int lzf_gpu_request_bucket(const uint8_t *op, const uint8_t *status,
                           const uint64_t *key_off, const uint32_t *key_len,
                           const uint64_t *val_off, const uint32_t *val_len, const int64_t *num, uint32_t n,
                           uint32_t *perm /* n */, uint32_t *slot /* n */,
                           uint32_t *class_first /* LZF_RQ_NCLASS + 1 */,
                           uint8_t *b_op, uint8_t *b_status, uint64_t *b_key_off, uint32_t *b_key_len,
                           uint64_t *b_val_off, uint32_t *b_val_len, int64_t *b_num,
                           void *work, void *stream);
int lzf_host_request_bucket(const uint8_t *op, const uint8_t *status,
                            const uint64_t *key_off, const uint32_t *key_len,
                            const uint64_t *val_off, const uint32_t *val_len, const int64_t *num, uint32_t n,
                            uint32_t *perm, uint32_t *slot, uint32_t *class_first,
                            uint8_t *b_op, uint8_t *b_status, uint64_t *b_key_off, uint32_t *b_key_len,
                            uint64_t *b_val_off, uint32_t *b_val_len, int64_t *b_num);
int lzf_gpu_request_stitch(const uint8_t *op, const uint8_t *status, const uint32_t *slot, uint32_t n,
                           const uint32_t *class_first /* device, LZF_RQ_NCLASS + 1 */,
                           const uint8_t *class_mode /* host, LZF_RQ_NCLASS */,
                           const uint64_t *class_base /* host, LZF_RQ_NCLASS */,
                           const uint64_t *b_rep_off, const uint32_t *b_rep_len,
                           const uint8_t *b_ent /* may be NULL */, const uint8_t *b_refused /* may be NULL */,
                           uint8_t *replies, uint64_t rep_cap, uint64_t code_base,
                           uint64_t *out_off /* n */, uint32_t *out_len /* n */, uint8_t *out_kind /* n */,
                           uint64_t *result /* 5 u64 */, void *stream);
int lzf_host_request_stitch(const uint8_t *op, const uint8_t *status, const uint32_t *slot, uint32_t n,
                            const uint32_t *class_first, const uint8_t *class_mode, const uint64_t *class_base,
                            const uint64_t *b_rep_off, const uint32_t *b_rep_len,
                            const uint8_t *b_ent, const uint8_t *b_refused,
                            uint8_t *replies, uint64_t rep_cap, uint64_t code_base,
                            uint64_t *out_off, uint32_t *out_len, uint8_t *out_kind, uint64_t *result);

/* Free the library's device scratch (all devices), the calling thread's and
 * the device workers' staging buffers; later calls allocate them again.
 * Each thread's staging buffers are also freed when the thread exits. */
void lzf_gpu_release(void);

/* One-time self-check of the current device (run lazily before the first
 * compress launch, or here): the table / lane / window compressor kernels
 * need the LDS to execute a wave's same-address ds_mskor_rtn_b32 in lane
 * order (gibson_amd/csrc/lzf_selfcheck.hip).  Returns 1 when that held (the
 * measured routing is used), 0 when it did not (compress batches then run
 * window64, which needs no ordering), or a negative LZF_GPU_E* code.  The
 * result also appears in lzf_gpu_kernel_info() as lds_order=... */
int lzf_gpu_selfcheck(void);
/* The probe itself, run again: mismatching lanes over 16 collision patterns
 * of 1024 waves (0 = lane order held), or a negative LZF_GPU_E* code. */
int lzf_gpu_lds_order_probe(void);

/* Which kernel generation the batch calls dispatch to (diagnostics):
 * returns a static string such as "compress=window64 decompress=tokpar". */
const char *lzf_gpu_kernel_info(void);

#ifdef __cplusplus
}
#endif

#endif /* LZF_GPU_H */
