/*
 * vfilter.h — C ABI of libvfilter_hip.so, the MI355X (gfx950) frame-filter backend.
 *
 * This library replaces the per-frame filter of kylemcdonald/distributed-video-filter:
 *
 *     inverted = cv2.bitwise_not(frame)            # inverter.py:41
 *
 * called once per frame from Worker.start()         # worker.py:57 -> inverter.py:29-46
 *
 * The reference is pure Python; its "FFI" for this path is the Python call into
 * OpenCV.  The build's Python side binds these entry points with ctypes
 * (distributed-video-filter_amd/vfilter/_lib.py); INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every entry point is extern "C", never throws, and returns an int status:
 *     VF_OK (0) on success, a negative VF_E_* code on failure;
 *   - the failing hipError_t and a human-readable message are kept per context
 *     (vf_last_error) and per thread for calls made without a context;
 *   - buffers are plain pointers and byte counts; any alignment and any byte count
 *     (including 0 and counts that are not a multiple of 16) are accepted;
 *   - HIP streams cross the boundary as `void*` (a hipStream_t; NULL = the null stream),
 *     so no HIP or torch type appears in a signature;
 *   - a context is bound to one device and is not thread-safe: one per worker process
 *     (the reference runs one filter per process, worker.py:5-28).
 *
 * Semantics of the filter (OpenCV `bitwise_not`, inverter.py:41): dst[i] = ~src[i] for
 * every byte of a C-contiguous uint8 H x W x 3 frame.  The operation is channel-order
 * agnostic (BGR vs RGB irrelevant) and shape agnostic, so a batch of frames packed back
 * to back is filtered as one byte range.
 */
#ifndef VFILTER_H
#define VFILTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VF_ABI_VERSION 3

/* status codes */
#define VF_OK           0
#define VF_E_INVALID   -1  /* bad argument (NULL pointer, negative count, size > capacity) */
#define VF_E_HIP       -2  /* a HIP runtime call failed; see vf_last_error / vf_last_hip_error */
#define VF_E_NOMEM     -3  /* host or device allocation failed */
#define VF_E_NODEVICE  -4  /* no usable gfx950 device / bad device ordinal */
#define VF_E_JPEG      -5  /* malformed, truncated or unsupported JPEG stream */

typedef struct vf_ctx vf_ctx;

/* ---- library / context ------------------------------------------------------------ */

/* ABI version of the loaded library (VF_ABI_VERSION).  Makes no HIP call. */
int vf_get_abi_version(void);

/* Static string for a VF_* status code.  Makes no HIP call. */
const char *vf_status_string(int status);

/* Number of visible HIP devices (0 when there is no GPU; never fails for that). */
int vf_device_count(int *out_count);

/* PCI address of HIP device `device` ("dddd:bb:dd.f", from hipDeviceGetPCIBusId) in `buf`
 * (`len` >= 13 bytes).  The host side reads the device's NUMA node from sysfs with it and
 * places that GPU worker's shared-memory frame ring on the node (the reference's workers keep
 * no host buffers of their own: frames arrive in pyzmq messages, worker.py:50-51). */
int vf_device_pci_bus_id(int device, char *buf, int len);

/* Create a context on `device`.  Allocates the pinned host staging ring and device slot
 * buffers used by the host->host entry points (VF_SLOTS slots, default 4, each of
 * min(`max_frame_bytes` x `max_batch`, 16 MiB) bytes; VF_SLOT_BYTES overrides, clamped to
 * [1 MiB, 64 MiB]) and two HIP streams (H2D + kernel, D2H: one SDMA engine per direction).
 * Replaces the per-process filter state of InverterWorker.__init__ (inverter.py:10-20). */
int vf_create(int device, size_t max_frame_bytes, int max_batch, vf_ctx **out);

/* Destroy a context (NULL is allowed).  Synchronises its streams first. */
int vf_destroy(vf_ctx *ctx);

/* Last error message of `ctx`, or of the calling thread when ctx is NULL.  Never NULL.
 * Every failing call also records its message for the calling thread, so a caller that
 * shares one context between threads (JPEG calls lease separate codecs) should read
 * vf_last_error(NULL) on the thread that saw the failure. */
const char *vf_last_error(const vf_ctx *ctx);

/* Last hipError_t recorded by `ctx` (0 if none), or by the calling thread when ctx is NULL. */
int vf_last_hip_error(const vf_ctx *ctx);

/* Device ordinal of the context. */
int vf_ctx_device(const vf_ctx *ctx, int *out_device);

/* ---- host -> host filtering (synchronous) ------------------------------------------- */

/* Invert `nbytes` bytes of host memory: dst[i] = ~src[i].
 * Replaces `cv2.bitwise_not(frame)` (inverter.py:41) for one frame.  `src` and `dst` may
 * be pageable or pinned, any alignment; they must not partially overlap (src == dst is
 * allowed).  Returns when dst is complete.  Paths: when both ranges lie inside page-locked
 * memory noted by vf_alloc_host / vf_host_register, ONE kernel launch reads src and writes
 * dst over PCIe in place (zero-copy: no HBM staging; 48.5 GB/s each way at 1080p x 32, the
 * same as two SDMA copies at once); otherwise H2D || kernel || D2H run pipelined over the
 * context's staging slots (other page-locked memory is DMA'd directly, pageable memory is
 * staged).  VF_ZEROCOPY=0 in the environment at vf_create turns the zero-copy path off. */
int vf_invert_host(vf_ctx *ctx, const uint8_t *src, uint8_t *dst, size_t nbytes);

/* Invert a batch of `n` frames of `frame_bytes` each, packed back to back in `src`;
 * results packed the same way in `dst`.  Replaces the per-frame loop
 * worker.py:35-57 -> inverter.py:41 for a batch.  Same rules as vf_invert_host. */
int vf_invert_batch_host(vf_ctx *ctx, const uint8_t *src, uint8_t *dst,
                         size_t frame_bytes, int n);

/* Invert `n` separately allocated frames (srcs[i] -> dsts[i], nbytes[i] bytes each; sizes
 * may differ, e.g. a mixed 480p/1080p/4K batch).  Frames in page-locked, device-mapped
 * memory are inverted by one launch per 64 frames, all at once (zero-copy); others are
 * gathered into the staging slots, filtered with one launch per slot and scattered back, so
 * small frames are not paid for one launch each.  Frames are independent: one frame's
 * destination must not overlap another frame's source or destination (a frame's own src and
 * dst may be equal).  Replaces worker.py:50-57 + inverter.py:29-46 for a batch of raw
 * frames. */
int vf_invert_frames_host(vf_ctx *ctx, const uint8_t *const *srcs, uint8_t *const *dsts,
                          const size_t *nbytes, int n);

/* ---- host -> host, asynchronous ------------------------------------------------------ */

/* Queue the filter for `n` frames (srcs[i] -> dsts[i], nbytes[i] each) and return at once
 * with a ticket (> 0); the asynchronous form of vf_invert_frames_host (worker.py:57).  The
 * context's engine thread streams queued batches through its slot ring back to back, so a
 * worker can receive its next batch while this one moves.  The caller keeps every buffer
 * alive and untouched until vf_wait(ticket) returns.  Page-locked buffers (vf_alloc_host,
 * vf_host_register, e.g. a shared-memory frame ring) are inverted in place over PCIe by one
 * launch per 64 frames on the context's zero-copy stream; pageable ones are staged through
 * the slot ring.  Tickets of the two paths may complete in either order. */
int vf_invert_frames_async(vf_ctx *ctx, const uint8_t *const *srcs, uint8_t *const *dsts,
                           const size_t *nbytes, int n, uint64_t *ticket);

/* Block until submission `ticket` has completed (its last D2H landed) and return its status.
 * *gpu_ms (may be NULL) gets its device time from first H2D to last D2H (-1 if unknown).
 * Also sets what vf_elapsed_ms / vf_last_timeline report. */
int vf_wait(vf_ctx *ctx, uint64_t ticket, float *gpu_ms);

/* *done = 1 if submission `ticket` has completed, else 0 (never blocks). */
int vf_query(vf_ctx *ctx, uint64_t ticket, int *done);

/* ---- device-resident filtering (asynchronous) -------------------------------------- */

/* Enqueue the invert kernel on `stream` over device memory: ddst[i] = ~dsrc[i].
 * Returns after the launch (does not synchronise).  Kernel-only path used by benchmarks
 * and by callers that keep frames resident in HBM. */
int vf_invert_device(vf_ctx *ctx, const void *dsrc, void *ddst, size_t nbytes, void *stream);

/* Enqueue one launch over `n` device frames given by device-memory descriptor arrays
 * (dsrcs/ddsts/nbytes are themselves arrays in DEVICE memory, n entries each).  For
 * HBM-resident frame pools whose frames are not contiguous. */
int vf_invert_device_frames(vf_ctx *ctx, const void *const *dsrcs, void *const *ddsts,
                            const size_t *nbytes, int n, size_t total_bytes, void *stream);

/* ---- memory helpers --------------------------------------------------------------- */

int vf_alloc_device(vf_ctx *ctx, size_t nbytes, void **out);
int vf_free_device(vf_ctx *ctx, void *p);
/* page-locked host memory (DMA-able without staging) */
int vf_alloc_host(vf_ctx *ctx, size_t nbytes, void **out);
int vf_free_host(vf_ctx *ctx, void *p);
/* page-lock an existing host range (e.g. a shared-memory frame ring) in place */
int vf_host_register(vf_ctx *ctx, void *p, size_t nbytes);
int vf_host_unregister(vf_ctx *ctx, void *p);
/* asynchronous copies on `stream` (synchronous w.r.t. the host if the host side is pageable) */
int vf_upload(vf_ctx *ctx, void *ddst, const void *hsrc, size_t nbytes, void *stream);
int vf_download(vf_ctx *ctx, void *hdst, const void *dsrc, size_t nbytes, void *stream);
int vf_memset_device(vf_ctx *ctx, void *d, int value, size_t nbytes, void *stream);
/* wait for `stream` (NULL = every stream of the context and the device) */
int vf_sync(vf_ctx *ctx, void *stream);

/* ---- timing ----------------------------------------------------------------------- */

/* Sum of kernel durations (ms, hipEvents) of the last host->host call on ctx. */
int vf_elapsed_ms(const vf_ctx *ctx, float *out_ms);

/* Per-chunk GPU timeline of the last host->host call (for Perfetto spans, the GPU side of
 * the reference's trace export, distributor.py:63-171).  For chunk i < min(n, max_chunks):
 * out4[4i..4i+3] = {H2D start, kernel start, kernel end, D2H end} in ms after the call's
 * start event, chunk_bytes[i] = its size (either array may be NULL).  *n_chunks = n.
 * A zero-copy call reports one record {0, 0, t, t}: one launch moved every byte. */
int vf_last_timeline(const vf_ctx *ctx, float *out4, size_t *chunk_bytes, int max_chunks,
                     int *n_chunks);

/* Benchmark loop over HBM-resident buffers: for step s in [0, steps) launch the invert
 * kernel from srcs[s % nbuf] to dsts[s % nbuf] (`nbytes` each, host arrays of device
 * pointers) back to back on `stream`, then synchronise.  A hipEvent pair brackets the whole
 * sequence; its duration (ms) goes to *region_ms (may be NULL).  If per_launch_ms is not
 * NULL, an extra event pair is recorded around every launch and each launch's duration goes
 * to per_launch_ms[s] (the pairs add a few microseconds of gap per launch).  The region pair
 * belongs to the context and is created by its first call (so a timed call only records,
 * launches and synchronises): calls on one context must not overlap. */
int vf_bench_device_ring(vf_ctx *ctx, void *const *srcs, void *const *dsts, int nbuf,
                         size_t nbytes, int steps, void *stream, float *per_launch_ms,
                         float *region_ms);


/* ---- JPEG: the reference's default mode (use_jpeg=True) ------------------------------
 *
 * With use_jpeg=True (the default, inverter.py:10) every frame travels as a JPEG made by
 * PyTurboJPEG (webcam_app.py:110), and the worker runs
 *     frame = self.jpeg.decode(frame_bytes)     # inverter.py:32
 *     inverted = cv2.bitwise_not(frame)         # inverter.py:41
 *     return self.jpeg.encode(inverted)         # inverter.py:44
 * with PyTurboJPEG's defaults (quality 85, TJSAMP_422, TJPF_BGR, flags 0).  These entry
 * points replace those TurboJPEG calls (tjDecompressHeader3 / tjDecompress2 / tjCompress2)
 * with a gfx950 baseline-JPEG codec whose integer arithmetic is libjpeg-turbo's: outputs are
 * bit-exact with libjpeg-turbo.  Constants below are TurboJPEG's (turbojpeg.h).
 * Supported: 8-bit baseline / extended-sequential Huffman JPEG, 1 or 3 components, one
 * interleaved scan, any Huffman tables, with or without restart intervals (DRI / RSTn)
 * (decode); TJSAMP_444/422/420/GRAY/440 (encode).
 * Anything else returns VF_E_JPEG with a message. */
#define VF_TJPF_RGB 0
#define VF_TJPF_BGR 1
#define VF_TJSAMP_444 0
#define VF_TJSAMP_422 1
#define VF_TJSAMP_420 2
#define VF_TJSAMP_GRAY 3
#define VF_TJSAMP_440 4
#define VF_TJFLAG_FASTUPSAMPLE 256   /* replicate chroma instead of fancy upsampling */
#define VF_TJFLAG_FASTDCT 2048       /* "ifast" forward DCT (else the accurate "islow") */
#define VF_TJFLAG_ACCURATEDCT 4096   /* accepted; islow is the default */

/* Header of one JPEG, no GPU work (replaces TurboJPEG.decode_header).  *subsamp = TJSAMP_*
 * (-1 if none matches), *colorspace = TJCS_YCbCr (1), TJCS_GRAY (2), or TJCS_RGB (0) for a
 * three-component stream libjpeg reads as RGB, which the decode calls refuse. */
int vf_jpeg_header(const uint8_t *jpeg, size_t size, int *width, int *height, int *subsamp,
                   int *colorspace);

/* Decoder frame-size limit of the context: a JPEG whose SOF claims more than max_pixels
 * (width x height) is refused with VF_E_JPEG before anything is sized from it, as is any side
 * above 65500 (libjpeg's JPEG_MAX_DIMENSION, jdinput.c initial_setup).  0 restores the
 * default, 8192 x 8192.  The frames a worker decodes come off the network
 * (inverter.py:31-32): without a limit, a few hundred bytes of header could ask the codec for
 * tens of GB.  Replaces no reference call (libjpeg-turbo applies only the per-side limit). */
int vf_jpeg_set_max_pixels(vf_ctx *ctx, uint64_t max_pixels);

/* Worst-case size of a vf_jpeg_encode output (tjBufSize); 0 for bad arguments. */
size_t vf_jpeg_buffer_size(int width, int height, int subsamp);

/* Encode n images (inverter.py:44, webcam_app.py:110): imgs[i] is an interleaved 8-bit
 * heights[i] x widths[i] x 3 image in pixel_format; outs[i] receives the JPEG (caps[i]
 * bytes available), sizes[i] its length.  One batched pass on the GPU. */
int vf_jpeg_encode(vf_ctx *ctx, const uint8_t *const *imgs, const int *widths, const int *heights,
                   int n, int pixel_format, int quality, int subsamp, int flags,
                   uint8_t *const *outs, const size_t *caps, size_t *sizes);

/* Decode n JPEGs (inverter.py:32, webcam_app.py:140) into interleaved 8-bit pixels
 * (outs[i] holds width x height x 3 bytes, caps[i] available). */
int vf_jpeg_decode(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                   int pixel_format, int flags, uint8_t *const *outs, const size_t *caps);

/* The whole default-mode filter for n frames on the GPU: decode -> bitwise_not -> encode
 * (inverter.py:32 -> :41 -> :44) with no host round trip of the pixels.  outs[i] receives
 * the inverted JPEG (caps[i] bytes available), sizes[i] its length. */
int vf_jpeg_invert(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                   int quality, int subsamp, int flags, uint8_t *const *outs, const size_t *caps,
                   size_t *sizes);

/* vf_jpeg_invert in three steps, so one host thread keeps batches in flight (the worker loop
 * of worker.py:35-76 receiving batch k+1 while batch k is on the GPU) instead of blocking per
 * batch:
 *   vf_jpeg_invert_submit  parses and stages the batch and queues all of its GPU work; returns
 *                          a ticket without waiting for the GPU.  The inputs are copied: the
 *                          caller may reuse them at once.  Each in-flight batch holds one of the
 *                          context's codecs (at most 8 in flight; never blocks);
 *   vf_jpeg_invert_query   *done = 1 once the batch's results have landed in host memory;
 *   vf_jpeg_invert_wait    blocks until then; *total = bytes of the packed outputs (frames
 *                          back to back, 64-B aligned).  A failed batch ends here (ticket gone);
 *   vf_jpeg_invert_fetch   copies the packed outputs to `out` (cap >= total; frame i is
 *                          sizes[i] bytes at offsets[i]) and ends the batch.  out == NULL ends
 *                          it without copying.  VF_E_INVALID with cap too small keeps it.
 * Same results as vf_jpeg_invert, bit for bit. */
int vf_jpeg_invert_submit(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                          int quality, int subsamp, int flags, uint64_t *ticket);
int vf_jpeg_invert_query(vf_ctx *ctx, uint64_t ticket, int *done);
int vf_jpeg_invert_wait(vf_ctx *ctx, uint64_t ticket, size_t *total);
int vf_jpeg_invert_fetch(vf_ctx *ctx, uint64_t ticket, uint8_t *out, size_t cap, size_t *sizes,
                         size_t *offsets);

/* After vf_jpeg_invert_wait: frame i's inverted JPEG straight into outs[i] when outs[i] is not
 * NULL and the JPEG fits caps[i] (e.g. the output half of the frame's shared-memory ring slot),
 * so the caller needs no packed buffer and no second copy.  sizes[i] = frame i's size either
 * way; *placed = how many frames were copied.  The batch stays open: release it with
 * vf_jpeg_invert_fetch(ctx, ticket, NULL, 0, NULL, NULL), or fetch the frames that did not
 * fit with a packed buffer first. */
int vf_jpeg_invert_scatter(vf_ctx *ctx, uint64_t ticket, uint8_t *const *outs, const size_t *caps,
                           size_t *sizes, int *placed);

/* Benchmark: the GPU part of vf_jpeg_invert (inputs already in HBM) run `iters` times; *ms =
 * mean wall ms per iteration; stage_ms (may be NULL, 8 floats) = mean ms of unstuff, Huffman
 * sync, Huffman write, DC+IDCT, colour+invert, FDCT+Huffman encode, byte stuffing, and the
 * mean number of sync passes. */
int vf_jpeg_bench_invert(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                         int quality, int subsamp, int flags, int iters, float *ms, float *stage_ms);

/* ---- another filter: a 256-entry table per channel (cv2.LUT) --------------------------
 *
 * Every per-pixel filter a plugin may put where the reference has cv2.bitwise_not
 * (inverter.py:41) -- gamma, levels, threshold, posterize, per-channel curves -- is
 * cv2.LUT(frame, table).  One table convention everywhere: `table` is channels x 256 bytes,
 * planar, table[c * 256 + v] = the output of value v in channel c, channels 1 or 3.  With one
 * channel every byte goes through the one table; with three the data is interleaved 3-channel,
 * a frame starts at channel 0 and its byte i uses table i % 3.  On the JPEG path channel c is
 * channel c of the decoded BGR pixel (inverter.py:32), so table[0..255] is applied to B.
 * `table` is a HOST pointer, read during the call only.  A NULL table, any other `channels`, or
 * (channels == 3) a frame whose size is not a multiple of 3 is VF_E_INVALID. */

/* Enqueue the table kernel on `stream` over device memory, the frame starting at channel 0.
 * Returns after the launch (does not synchronise); any alignment; dsrc == ddst is allowed. */
int vf_lut_device(vf_ctx *ctx, const void *dsrc, void *ddst, size_t nbytes,
                  const uint8_t *table, int channels, void *stream);

/* The filter on `n` separately allocated host frames (srcs[i] -> dsts[i], nbytes[i] each),
 * synchronous: upload, kernel, download on a stream of the context.  Pageable or page-locked
 * memory at any alignment, srcs[i] == dsts[i] allowed, frames independent as for
 * vf_invert_frames_host.  Frames larger than the context's staging are cut (mid-pixel if need
 * be).  Not pipelined: the zero-copy and asynchronous paths are vf_invert_*'s alone. */
int vf_lut_frames_host(vf_ctx *ctx, const uint8_t *const *srcs, uint8_t *const *dsts,
                       const size_t *nbytes, int n, const uint8_t *table, int channels);

/* vf_jpeg_invert with the table in place of the inversion: decode -> cv2.LUT -> encode. */
int vf_jpeg_lut(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                const uint8_t *table, int channels, int quality, int subsamp, int flags,
                uint8_t *const *outs, const size_t *caps, size_t *sizes);

/* vf_jpeg_invert_submit with the table (copied: the caller may reuse it at once).  The ticket
 * is an invert ticket: collect with vf_jpeg_invert_query / _wait / _fetch / _scatter. */
int vf_jpeg_lut_submit(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                       const uint8_t *table, int channels, int quality, int subsamp, int flags,
                       uint64_t *ticket);

/* vf_jpeg_bench_invert with the table in the colour stage. */
int vf_jpeg_bench_lut(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                      const uint8_t *table, int channels, int quality, int subsamp, int flags,
                      int iters, float *ms, float *stage_ms);

/* ---- 2-D convolution filter (cv2.filter2D) ------------------------------------------------
 * dst = cv2.filter2D(src, -1, K / 2^shift) for uint8 frames of 1 or 3 interleaved channels in
 * packed rows: correlation (no flip), anchor at the centre, exact integer arithmetic, the sum
 * rounded half to even and saturated to 0..255.  `weights` is a HOST pointer to
 * kw * kh int16, row-major, read during the call only; kw and kh are odd and at most 7,
 * 0 <= shift <= 16, sum|K| <= 65536.  `border` is one of VF_BORDER_*.  Anything else, a NULL
 * `weights`, `channels` other than 1 or 3, or a frame with width <= 0 or height <= 0 (other than
 * the empty 0 x 0 frame, which is skipped) is VF_E_INVALID. */
#define VF_BORDER_REFLECT101 0 /* cv2.BORDER_DEFAULT: gfedcb|abcdefgh|gfedcba */
#define VF_BORDER_REPLICATE  1 /* aaaaaa|abcdefgh|hhhhhhh */
#define VF_BORDER_CONSTANT   2 /* 000000|abcdefgh|0000000 (the constant is 0) */

/* Enqueue the convolution on `stream` over device memory (width * height * channels bytes
 * each).  Returns after the launch (does not synchronise); any alignment.  Out of place only:
 * ranges that overlap are VF_E_INVALID. */
int vf_conv_device(vf_ctx *ctx, const void *dsrc, void *ddst, int width, int height, int channels,
                   const int16_t *weights, int kw, int kh, int shift, int border, void *stream);

/* The filter on `n` separately allocated host frames (srcs[i] -> dsts[i], widths[i] x heights[i]
 * x channels), synchronous: upload, kernel, download on a stream of the context.  srcs[i] ==
 * dsts[i] is allowed.  A frame larger than the context's staging is cut into bands of rows with
 * their halo; VF_E_INVALID when kh rows of a frame do not fit it. */
int vf_conv_frames_host(vf_ctx *ctx, const uint8_t *const *srcs, uint8_t *const *dsts,
                        const int *widths, const int *heights, int n, int channels,
                        const int16_t *weights, int kw, int kh, int shift, int border);

/* vf_jpeg_invert with the convolution in place of the inversion: decode -> cv2.filter2D ->
 * encode on the GPU; channel c of the kernel's view is channel c of the decoded BGR frame. */
int vf_jpeg_conv(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                 const int16_t *weights, int kw, int kh, int shift, int border, int quality,
                 int subsamp, int flags, uint8_t *const *outs, const size_t *caps, size_t *sizes);

/* vf_jpeg_invert_submit with the convolution (weights copied).  The ticket is an invert
 * ticket: collect with vf_jpeg_invert_query / _wait / _fetch / _scatter. */
int vf_jpeg_conv_submit(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                        const int16_t *weights, int kw, int kh, int shift, int border, int quality,
                        int subsamp, int flags, uint64_t *ticket);

/* vf_jpeg_bench_invert with the convolution between the decode and the encode. */
int vf_jpeg_bench_conv(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                       const int16_t *weights, int kw, int kh, int shift, int border, int quality,
                       int subsamp, int flags, int iters, float *ms, float *stage_ms);

/* ---- rank filters (cv2.erode, cv2.dilate, cv2.medianBlur) ----------------------------------
 * For uint8 frames of 1 or 3 interleaved channels in packed rows, every channel on its own, exact
 * (DESIGN.md 18).  `element` is a HOST pointer to kw * kh bytes, row-major (kh rows of kw), read
 * during the call only; non-zero means "member".  kw and kh are odd and at most 7, at least one
 * member; the anchor is the centre and offsets are not reflected.
 *   VF_RANK_ERODE   the minimum over the members' taps, 255 when no tap resolves to a pixel
 *   VF_RANK_DILATE  the maximum over them, 0 when none does
 *   VF_RANK_MEDIAN  the median of the full square: kw == kh in {3, 5}, every entry non-zero, and
 *                   `border` VF_BORDER_REPLICATE (cv2.medianBlur has no other)
 * `border` is one of VF_BORDER_*.  For erode and dilate VF_BORDER_CONSTANT is cv2's default
 * border: a tap outside the frame is left out of the set (NOT read as 0, unlike vf_conv_*).
 * Anything else, a NULL `element`, `channels` other than 1 or 3, or a frame with width <= 0 or
 * height <= 0 (other than the empty 0 x 0 frame, which is skipped) is VF_E_INVALID. */
#define VF_RANK_ERODE  0
#define VF_RANK_DILATE 1
#define VF_RANK_MEDIAN 2

/* Enqueue the filter on `stream` over device memory (width * height * channels bytes each).
 * Returns after the launch (does not synchronise); any alignment.  Out of place only: ranges
 * that overlap are VF_E_INVALID. */
int vf_rank_device(vf_ctx *ctx, const void *dsrc, void *ddst, int width, int height, int channels,
                   int op, const uint8_t *element, int kw, int kh, int border, void *stream);

/* The filter on `n` separately allocated host frames (srcs[i] -> dsts[i], widths[i] x heights[i]
 * x channels), synchronous, as vf_conv_frames_host: srcs[i] == dsts[i] is allowed; a frame larger
 * than the context's staging is cut into bands of rows with their halo; VF_E_INVALID when kh rows
 * of a frame do not fit it. */
int vf_rank_frames_host(vf_ctx *ctx, const uint8_t *const *srcs, uint8_t *const *dsts,
                        const int *widths, const int *heights, int n, int channels, int op,
                        const uint8_t *element, int kw, int kh, int border);

/* vf_jpeg_invert with the rank filter in place of the inversion: decode -> filter -> encode on
 * the GPU, on each channel of the decoded BGR frame. */
int vf_jpeg_rank(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n, int op,
                 const uint8_t *element, int kw, int kh, int border, int quality, int subsamp,
                 int flags, uint8_t *const *outs, const size_t *caps, size_t *sizes);

/* vf_jpeg_invert_submit with the rank filter (element copied).  The ticket is an invert ticket:
 * collect with vf_jpeg_invert_query / _wait / _fetch / _scatter. */
int vf_jpeg_rank_submit(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                        int op, const uint8_t *element, int kw, int kh, int border, int quality,
                        int subsamp, int flags, uint64_t *ticket);

/* vf_jpeg_bench_invert with the rank filter between the decode and the encode. */
int vf_jpeg_bench_rank(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                       int op, const uint8_t *element, int kw, int kh, int border, int quality,
                       int subsamp, int flags, int iters, float *ms, float *stage_ms);

/* ---- colour matrix (cv2.transform: grayscale, BGR <-> RGB, sepia, saturation, ...) -----------
 * For uint8 frames of 3 interleaved channels, exact in integers.  `matrix` is a
 * HOST pointer to 12 int32, row-major [M | t] 3 x 4, read during the call only:
 *   acc[c] = sum_k M[c][k] * src[k] + t[c]          c, k in {0, 1, 2}
 *   q      = acc                                     when shift == 0, else acc / 2^shift rounded:
 *              VF_ROUND_HALF_EVEN  to nearest, a tie to the even integer
 *              VF_ROUND_HALF_UP    (acc + 2^(shift - 1)) >> shift, the shift arithmetic
 *   dst[c] = min(max(q, 0), 255)
 * Every M[c][k] fits int16, sum_k |M[c][k]| <= 65536 per row, 0 <= shift <= 16 and t[c], already
 * scaled by 2^shift, has |t[c]| <= 255 * 2^shift.  Anything else, a NULL `matrix`, an unknown
 * rounding, or 1-channel frames is VF_E_INVALID. */
#define VF_ROUND_HALF_EVEN 0
#define VF_ROUND_HALF_UP   1

/* The bytes of one workgroup's tile of the colour-matrix kernel (a multiple of 48).  Makes no
 * HIP call. */
size_t vf_mix_tile_bytes(void);

/* Enqueue the matrix on `stream` over nbytes of device memory, whole 3-byte pixels
 * (nbytes % 3 == 0).  Returns after the launch (does not synchronise); any alignment.  ddst ==
 * dsrc exactly is allowed; a partial overlap is VF_E_INVALID.  nbytes == 0 writes nothing. */
int vf_mix_device(vf_ctx *ctx, const void *dsrc, void *ddst, size_t nbytes, const int32_t *matrix,
                  int shift, int rounding, void *stream);

/* The matrix on `n` separately allocated host frames (srcs[i] -> dsts[i], widths[i] x heights[i]
 * x channels, channels == 3), synchronous, as vf_conv_frames_host: srcs[i] == dsts[i] is allowed;
 * a frame larger than the context's staging is cut into bands of rows. */
int vf_mix_frames_host(vf_ctx *ctx, const uint8_t *const *srcs, uint8_t *const *dsts,
                       const int *widths, const int *heights, int n, int channels,
                       const int32_t *matrix, int shift, int rounding);

/* vf_jpeg_invert with the matrix in place of the inversion: decode -> matrix -> encode on the
 * GPU, on the pixels of the decoded BGR frame (channel 0 is blue). */
int vf_jpeg_mix(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                const int32_t *matrix, int shift, int rounding, int quality, int subsamp, int flags,
                uint8_t *const *outs, const size_t *caps, size_t *sizes);

/* vf_jpeg_invert_submit with the matrix (copied).  The ticket is an invert ticket: collect with
 * vf_jpeg_invert_query / _wait / _fetch / _scatter. */
int vf_jpeg_mix_submit(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                       const int32_t *matrix, int shift, int rounding, int quality, int subsamp,
                       int flags, uint64_t *ticket);

/* vf_jpeg_bench_invert with the matrix between the decode and the encode. */
int vf_jpeg_bench_mix(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                      const int32_t *matrix, int shift, int rounding, int quality, int subsamp,
                      int flags, int iters, float *ms, float *stage_ms);

/* ---- separable filter (cv2.sepFilter2D, cv2.blur, cv2.boxFilter, wide Gaussians) -------------
 * For uint8 frames of 1 or 3 interleaved channels, exact in integers.  `kx` holds
 * `kw` horizontal taps and `ky` `kh` vertical taps, int16, HOST pointers read during the call
 * only; kw and kh are odd and at most 31, the anchor is the centre, the operation correlation:
 *   acc = sum_j ky[j] * sum_i kx[i] * src[by(y + j - kh/2)][bx(x + i - kw/2)]   exact, 32-bit
 *   q   = acc                                  shift == 0 and divisor == 1
 *       = acc / 2^shift rounded                0 < shift <= 16: VF_ROUND_HALF_EVEN or VF_ROUND_HALF_UP
 *       = floor((2 acc + d) / (2 d))           divisor d, odd, 1 < d <= 1023: to nearest (no tie exists)
 *   dst = min(max(q, 0), 255)
 * which is vf_conv_* with the kernel outer(ky, kx) wherever both exist.  sum|kx| * sum|ky| <=
 * 65536; `divisor` is 1 for none, and a shift and a divisor exclude each other; `border` is a
 * VF_BORDER_*.  cv2.blur(src, (w, h)): all taps 1, divisor w * h.  Anything else, NULL taps, an
 * unknown rounding or border is VF_E_INVALID with the reason, before any GPU work. */

/* The output tile of one workgroup of the separable kernel for kw x kh taps: *row_bytes bytes
 * of *rows rows.  Makes no HIP call.  VF_E_INVALID for tap counts the filter refuses. */
int vf_sep_tile(int kw, int kh, int *row_bytes, int *rows);

/* Enqueue the filter on `stream` over one device-resident frame, as vf_conv_device: out of place
 * (src and dst must not overlap), any alignment, returns after the launch. */
int vf_sep_device(vf_ctx *ctx, const void *dsrc, void *ddst, int width, int height, int channels,
                  const int16_t *kx, int kw, const int16_t *ky, int kh, int shift, int divisor,
                  int rounding, int border, void *stream);

/* The filter on `n` separately allocated host frames, synchronous, as vf_conv_frames_host:
 * srcs[i] == dsts[i] is allowed; a frame larger than the context's staging is cut into bands of
 * rows with halos of kh / 2 rows. */
int vf_sep_frames_host(vf_ctx *ctx, const uint8_t *const *srcs, uint8_t *const *dsts,
                       const int *widths, const int *heights, int n, int channels,
                       const int16_t *kx, int kw, const int16_t *ky, int kh, int shift,
                       int divisor, int rounding, int border);

/* vf_jpeg_invert with the filter in place of the inversion: decode -> filter -> encode on the
 * GPU, on the decoded BGR frame. */
int vf_jpeg_sep(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                const int16_t *kx, int kw, const int16_t *ky, int kh, int shift, int divisor,
                int rounding, int border, int quality, int subsamp, int flags,
                uint8_t *const *outs, const size_t *caps, size_t *sizes);

/* vf_jpeg_invert_submit with the filter (the taps are copied).  The ticket is an invert ticket. */
int vf_jpeg_sep_submit(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                       const int16_t *kx, int kw, const int16_t *ky, int kh, int shift,
                       int divisor, int rounding, int border, int quality, int subsamp, int flags,
                       uint64_t *ticket);

/* vf_jpeg_bench_invert with the filter between the decode and the encode. */
int vf_jpeg_bench_sep(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                      const int16_t *kx, int kw, const int16_t *ky, int kh, int shift, int divisor,
                      int rounding, int border, int quality, int subsamp, int flags, int iters,
                      float *ms, float *stage_ms);

/* ---- level filter (cv2.equalizeHist, auto-levels) and the histogram ---------------------------
 * For uint8 frames of 1 or 3 interleaved channels, bit-exact.  Per frame: the
 * histogram of the frame, hist[c][v] = the bytes of channel c equal to v, as uint32; from it a
 * 256-entry table per channel by a fixed rule; the table applied.  A frame has at most 2^32 - 1
 * pixels.
 *   rule     VF_LEVEL_EQUALIZE: cv2.equalizeHist's table of a histogram h with `total` entries:
 *              i0 the first v with h[v] != 0; the identity when h[i0] == total; else
 *              scale = 255.0f / (float)(total - h[i0]), table[v] = 0 for v <= i0 and
 *              clamp(rint((float)(h[i0 + 1] + .. + h[v]) * scale), 0, 255) above, in IEEE single
 *              precision, every operation rounded to nearest even.
 *            VF_LEVEL_STRETCH: in integers, cut_lo = (total * clip_lo) >> 16, cut_hi likewise;
 *              lo the smallest v with h[0] + .. + h[v] > cut_lo, hi the largest v with
 *              h[v] + .. + h[255] > cut_hi; the identity when hi <= lo; else table[v] = 0 for
 *              v <= lo, 255 for v >= hi, (510 (v - lo) + (hi - lo)) / (2 (hi - lo)) between.
 *   mask     bits 0..2: the channels that are levelled, the others pass unchanged; 0: all of the
 *            frame's channels; a bit beyond the frame's channel count is refused.
 *   link     0: each masked channel its own table from its own histogram; 1: one table for all
 *            masked channels from the sum of their histograms (total: the sum of their pixel
 *            counts, which must fit 32 bits as well).
 *   clip_lo, clip_hi   0 .. 32767, in units of 1 / 65536 of the total; the stretch rule's, and 0
 *            for equalize.
 * Anything else is VF_E_INVALID with the reason, before any GPU work.  The empty frame is a no-op. */
#define VF_LEVEL_EQUALIZE 0
#define VF_LEVEL_STRETCH  1

/* Enqueue the histogram of `nbytes` device bytes (whole pixels: nbytes % channels == 0) on
 * `stream`: dhist, channels * 256 uint32 in device memory (4-byte aligned), is zeroed and
 * counted into.  Any alignment of dsrc; returns after the launch. */
int vf_hist_device(vf_ctx *ctx, const void *dsrc, size_t nbytes, int channels, uint32_t *dhist,
                   void *stream);

/* The histograms of `n` separately allocated host frames of mixed sizes, synchronous: hists
 * receives n * channels * 256 host uint32, frame i's at i * channels * 256.  A frame larger than
 * the context's staging is counted over several fills.  Each nbytes[i] % channels == 0. */
int vf_hist_frames_host(vf_ctx *ctx, const uint8_t *const *srcs, const size_t *nbytes, int n,
                        int channels, uint32_t *hists);

/* Enqueue the filter on `stream` over one device-resident frame: any alignment, ddst == dsrc
 * allowed (the histogram is complete before the first byte is written), a partial overlap is
 * not; returns after the launches.  The histogram words are the context's: calls on one context
 * that may run at the same time on different streams need a context each. */
int vf_level_device(vf_ctx *ctx, const void *dsrc, void *ddst, int width, int height, int channels,
                    int rule, int mask, int link, int clip_lo, int clip_hi, void *stream);

/* The filter on `n` separately allocated host frames of mixed sizes, synchronous; srcs[i] ==
 * dsts[i] is allowed.  A frame that does not fit the context's staging whole is refused: the
 * table needs the whole frame, so a frame is never cut into bands. */
int vf_level_frames_host(vf_ctx *ctx, const uint8_t *const *srcs, uint8_t *const *dsts,
                         const int *widths, const int *heights, int n, int channels, int rule,
                         int mask, int link, int clip_lo, int clip_hi);

/* vf_jpeg_invert with the filter in place of the inversion: decode -> level -> encode on the GPU,
 * on the decoded 3-channel BGR frame (grayscale inputs included), each frame from its own
 * histogram. */
int vf_jpeg_level(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                  int rule, int mask, int link, int clip_lo, int clip_hi, int quality, int subsamp,
                  int flags, uint8_t *const *outs, const size_t *caps, size_t *sizes);

/* vf_jpeg_invert_submit with the filter.  The ticket is an invert ticket. */
int vf_jpeg_level_submit(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                         int rule, int mask, int link, int clip_lo, int clip_hi, int quality,
                         int subsamp, int flags, uint64_t *ticket);

/* vf_jpeg_bench_invert with the filter between the decode and the encode. */
int vf_jpeg_bench_level(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                        int rule, int mask, int link, int clip_lo, int clip_hi, int quality,
                        int subsamp, int flags, int iters, float *ms, float *stage_ms);

/* ---- CLAHE (cv2.createCLAHE(clipLimit, tileGridSize).apply) ------------------------------------
 * Contrast-limited adaptive histogram equalisation for uint8 frames of 1 or 3 interleaved
 * channels, bit-exact by the rule below (a transcription of OpenCV 4.x clahe.cpp for
 * 8-bit input; every float operation is one IEEE single-precision operation rounded to nearest
 * even, none fused).  A frame has at most 2^32 - 1 pixels and sides of at most 2^30.
 *   tiles_x, tiles_y   1 .. 16 each: cv2's tileGridSize = (x, y).
 *   clip_q8  the clip limit in units of 1 / 256, 0 .. 2^24; 0: no clipping.
 *   mask     bits 0..2: the channels that are filtered, each on its own, the others pass
 *            unchanged; 0: all of the frame's channels; a bit beyond the frame's channel count is
 *            refused.
 * Geometry: when W % tiles_x == 0 and H % tiles_y == 0 the extended frame is the frame; else it is
 * padded on the right by tiles_x - W % tiles_x and at the bottom by tiles_y - H % tiles_y (a full
 * tiles_x or tiles_y on an axis that divides, as cv2 does), reflecting without the edge pixel
 * (BORDER_REFLECT_101).  tw = We / tiles_x, th = He / tiles_y, area = tw * th, at most 2^31 - 1.
 * Per tile and channel: h[256] counts the tile's pixels; with clip_q8 > 0, clip =
 * max((clip_q8 * area) >> 16, 1), the excess above clip is cut off every bin and given back: every
 * bin gains excess / 256, and with residual = excess % 256 > 0 and step = max(256 / residual, 1)
 * bin v gains 1 when v % step == 0 and v / step < residual; scale = 255.0f / (float)area and
 * table[v] = clamp(rint((float)(h[0] + .. + h[v]) * scale), 0, 255).
 * Per pixel (y, x) with value s: txf = (float)x * (1.0f / (float)tw) - 0.5f, tx1 = floor(txf),
 * xa = txf - tx1, xa1 = 1.0f - xa, then tx2 = min(tx1 + 1, tiles_x - 1), tx1 = max(tx1, 0); the
 * same in y; dst = clamp(rint((T[ty1][tx1][s] * xa1 + T[ty1][tx2][s] * xa) * ya1 +
 * (T[ty2][tx1][s] * xa1 + T[ty2][tx2][s] * xa) * ya), 0, 255).
 * Anything else is VF_E_INVALID with the reason, before any GPU work.  The empty frame is a no-op. */

/* Enqueue the filter on `stream` over one device-resident frame: any alignment, ddst == dsrc
 * allowed (every table is complete before the first byte is written), a partial overlap is not;
 * returns after the launches.  The tile histograms and tables are the context's: calls on one
 * context that may run at the same time on different streams need a context each. */
int vf_clahe_device(vf_ctx *ctx, const void *dsrc, void *ddst, int width, int height, int channels,
                    int clip_q8, int tiles_x, int tiles_y, int mask, void *stream);

/* The filter on `n` separately allocated host frames of mixed sizes and one channel count,
 * synchronous; srcs[i] == dsts[i] is allowed.  A frame that does not fit the context's staging
 * whole is refused: the tables need the whole frame, so a frame is never cut into bands. */
int vf_clahe_frames_host(vf_ctx *ctx, const uint8_t *const *srcs, uint8_t *const *dsts,
                         const int *widths, const int *heights, int n, int channels, int clip_q8,
                         int tiles_x, int tiles_y, int mask);

/* vf_jpeg_invert with the filter in place of the inversion: decode -> CLAHE -> encode on the GPU,
 * on the decoded 3-channel BGR frame (grayscale inputs included). */
int vf_jpeg_clahe(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                  int clip_q8, int tiles_x, int tiles_y, int mask, int quality, int subsamp,
                  int flags, uint8_t *const *outs, const size_t *caps, size_t *sizes);

/* vf_jpeg_invert_submit with the filter.  The ticket is an invert ticket. */
int vf_jpeg_clahe_submit(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                         int clip_q8, int tiles_x, int tiles_y, int mask, int quality, int subsamp,
                         int flags, uint64_t *ticket);

/* vf_jpeg_bench_invert with the filter between the decode and the encode. */
int vf_jpeg_bench_clahe(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                        int clip_q8, int tiles_x, int tiles_y, int mask, int quality, int subsamp,
                        int flags, int iters, float *ms, float *stage_ms);

/* ---- the affine warp (cv2.warpAffine, cv2.flip) -------------------------------------------------
 * Every output pixel (y, x) of a uint8 frame of 1 or 3 interleaved channels reads the source at
 * sx = m0 x + m1 y + m2, sy = m3 x + m4 y + m5, m the map FROM DESTINATION TO SOURCE (cv2's
 * WARP_INVERSE_MAP form; cv2.invertAffineTransform of a forward map), in the fixed point of OpenCV
 * 3.x .. 4.10 imgwarp.cpp for 8-bit frames (bit-exact by the rule below).  The frame
 * keeps its size.
 *   m       six finite doubles; read when mode is 0.
 *   mode    0: the given m; 1: flip horizontal, 2: flip vertical, 3: both, resolved per frame of
 *           W x H to {-1, 0, W-1, 0, 1, 0}, {1, 0, 0, 0, -1, H-1} and {-1, 0, W-1, 0, -1, H-1}.
 *   interp  0: linear (cv2.INTER_LINEAR), 1: nearest (cv2.INTER_NEAREST).
 *   border  a VF_BORDER_*; value: three ints 0 .. 255, the constant border's byte per channel
 *           (cv2's borderValue; a 1-channel frame uses value[0]).
 * Every double operation is rounded separately, none fused; rint rounds half to even:
 *   adelta(x) = int(rint((m0 x) 1024)), bdelta(x) = int(rint((m3 x) 1024)),
 *   X0(y) = int(rint((m1 y + m2) 1024)) + rd, Y0(y) = int(rint((m4 y + m5) 1024)) + rd,
 *   rd = 16 for linear, 512 for nearest.
 * Linear: X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5 (arithmetic), sx = clamp(X >> 5, -32768,
 * 32767), fx = X & 31, the same in y; the taps (sy, sx), (sy, sx+1), (sy+1, sx), (sy+1, sx+1) weigh
 * 32 (32-fx)(32-fy), 32 fx (32-fy), 32 (32-fx) fy, 32 fx fy (sum 32768); dst = (sum + 16384) >> 15.
 * Nearest: sx = clamp((X0 + adelta) >> 10, -32768, 32767), the same in y; dst is the tap (sy, sx).
 * A tap: each axis goes through the border rule on its own; under VF_BORDER_CONSTANT a tap with
 * either index outside the frame is value[c], decided tap by tap.
 * Limits, VF_E_INVALID with the reason before any GPU work: sides of at most 32767; per frame
 * |m0| (W-1) 1024, |m3| (W-1) 1024 and |m1 y + m2| 1024 + 512 at y = 0 and y = H-1 (and the same
 * for m4, m5) each below 2^30.  The empty frame is a no-op. */

/* Enqueue the filter on `stream` over one device-resident frame: any alignment; ddst must not
 * overlap dsrc (an output pixel reads anywhere); returns after the launch. */
int vf_warp_device(vf_ctx *ctx, const void *dsrc, void *ddst, int width, int height, int channels,
                   const double *m, int mode, int interp, int border, const int *value,
                   void *stream);

/* The filter on `n` separately allocated host frames of mixed sizes and one channel count,
 * synchronous; srcs[i] == dsts[i] is allowed (the source is the staged copy).  A frame that does
 * not fit the context's staging whole is refused: a frame is never cut into bands. */
int vf_warp_frames_host(vf_ctx *ctx, const uint8_t *const *srcs, uint8_t *const *dsts,
                        const int *widths, const int *heights, int n, int channels,
                        const double *m, int mode, int interp, int border, const int *value);

/* vf_jpeg_invert with the filter in place of the inversion: decode -> warp -> encode on the GPU,
 * on the decoded 3-channel BGR frame (grayscale inputs included). */
int vf_jpeg_warp(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                 const double *m, int mode, int interp, int border, const int *value, int quality,
                 int subsamp, int flags, uint8_t *const *outs, const size_t *caps, size_t *sizes);

/* vf_jpeg_invert_submit with the filter.  The ticket is an invert ticket. */
int vf_jpeg_warp_submit(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                        const double *m, int mode, int interp, int border, const int *value,
                        int quality, int subsamp, int flags, uint64_t *ticket);

/* vf_jpeg_bench_invert with the filter between the decode and the encode. */
int vf_jpeg_bench_warp(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                       const double *m, int mode, int interp, int border, const int *value,
                       int quality, int subsamp, int flags, int iters, float *ms, float *stage_ms);

/* ---- the resize (cv2.resize) --------------------------------------------------------------------
 * A uint8 frame of W x H pixels of 1 or 3 interleaved channels becomes one of dw x dh: with dw and
 * dh not 0 that size, scale_x = 1.0 / ((double)dw / W); with both 0 and fx, fy finite and positive
 * dw = rint(W fx) (half to even), scale_x = 1.0 / fx, which is not W / dw.  The same in y.  Every
 * double and float operation is rounded separately, none fused (written from OpenCV
 * 3.x .. 4.10 resize.cpp's generic path, bit-exact by the rule below, which governs).
 *   VF_INTER_NEAREST  sx(dx) = min(floor(dx scale_x), W - 1), the same in y; dst = src[sy][sx].
 *   VF_INTER_LINEAR   per column f = (float)((dx + 0.5) scale_x - 0.5), sx = floor(f), f -= sx; sx < 0:
 *                     f = 0, sx = 0; sx >= W - 1: f = 0, sx = W - 1; a0 = rint((1.f - f) 2048.f), a1 =
 *                     rint(f 2048.f); the taps are columns sx and min(sx + 1, W - 1).  Per row the same
 *                     without the two resets: rows clamp(sy, 0, H - 1) and clamp(sy + 1, 0, H - 1) with
 *                     b0, b1 as they are.  In int32, h(r) = (S[r][sx] a0 + S[r][sx1] a1) >> 4 and
 *                     dst = (((b0 h(r0)) >> 16) + ((b1 h(r1)) >> 16) + 2) >> 2.
 *   VF_INTER_AREA     iscale_x = rint(scale_x); built where |scale_x - iscale_x| < DBL_EPSILON on both
 *                     axes and both factors are 1 .. 16: dst is the mean of the iscale_x x iscale_y
 *                     block at (dx iscale_x, dy iscale_y), (sum + 2) >> 2 at 2 x 2, else
 *                     sat(rint((float)sum * (1.f / (iscale_x iscale_y)))).  A block that overruns the
 *                     frame (the fx, fy form only: columns dx >= W / iscale_x, and every column of a
 *                     row block past H) is sat(rint((float)sum / count)) over its pixels inside.
 * Linear with both factors exactly 2 runs as area, as in cv2.  Limits, VF_E_INVALID with the reason
 * before any GPU work: sides of source and result 1 .. 32767; area at any other scale; cubic (2) and
 * Lanczos (4) are not built.  The empty frame is a no-op. */
#define VF_INTER_NEAREST 0
#define VF_INTER_LINEAR  1
#define VF_INTER_AREA    3

/* The size of the result for a frame of width x height.  No GPU work. */
int vf_resize_out_size(vf_ctx *ctx, int width, int height, int dw, int dh, double fx, double fy,
                       int interp, int *out_w, int *out_h);

/* Enqueue the filter on `stream` over one device-resident frame; ddst holds the result's size
 * (ask the function above): any alignment; ddst must not overlap dsrc at all; returns after the launch. */
int vf_resize_device(vf_ctx *ctx, const void *dsrc, void *ddst, int width, int height, int channels,
                     int dw, int dh, double fx, double fy, int interp, void *stream);

/* The filter on `n` separately allocated host frames of mixed sizes and one channel count,
 * synchronous; dsts[i] holds frame i's result size, and must not overlap srcs[i] unless the two
 * sizes are equal.  A frame or a result that does not fit the context's staging whole is refused:
 * a frame is never cut into bands. */
int vf_resize_frames_host(vf_ctx *ctx, const uint8_t *const *srcs, uint8_t *const *dsts,
                          const int *widths, const int *heights, int n, int channels, int dw,
                          int dh, double fx, double fy, int interp);

/* vf_jpeg_invert with the filter in place of the inversion: decode -> resize -> encode on the GPU,
 * on the decoded 3-channel BGR frame (grayscale inputs included).  Every output JPEG has its
 * frame's RESULT size (header, MCU padding and block counts follow it); a batch may mix input
 * sizes, and with fx, fy each frame is scaled from its own size. */
int vf_jpeg_resize(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                   int dw, int dh, double fx, double fy, int interp, int quality, int subsamp,
                   int flags, uint8_t *const *outs, const size_t *caps, size_t *sizes);

/* vf_jpeg_invert_submit with the filter.  The ticket is an invert ticket. */
int vf_jpeg_resize_submit(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes,
                          int n, int dw, int dh, double fx, double fy, int interp, int quality,
                          int subsamp, int flags, uint64_t *ticket);

/* vf_jpeg_bench_invert with the filter between the decode and the encode. */
int vf_jpeg_bench_resize(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                         int dw, int dh, double fx, double fy, int interp, int quality,
                         int subsamp, int flags, int iters, float *ms, float *stage_ms);

/* ---- filter chains (cv2.morphologyEx, difference of blurs, ...) -----------------------------
 * A program is a straight-line list of 1 .. VF_CHAIN_MAX_STEPS steps over values.
 * Value 0 is the input frame (uint8, 1 or 3 interleaved channels, packed rows), value i the result
 * of step i (1-based), and the program's result is the last step's value.  Each step names its
 * operand `a`, a binary step `b` as well; operands are earlier values.  Every step sees
 * whole-frame borders, so the result is exactly what running the steps one after the other on
 * whole frames gives.  Step kinds:
 *   VF_STEP_TABLE   cv2.LUT: `data` is channels x 256 bytes, planar (as for vf_lut_*)
 *   VF_STEP_CONV    cv2.filter2D: `data` is kw * kh int16 weights, with `shift` and `border`
 *   VF_STEP_RANK    `op` a VF_RANK_*: `data` is the kw * kh element bytes, with `border`
 *   VF_STEP_BINARY  `op` a VF_BIN_*, per byte on the values `a` and `b`:
 *                   SUBTRACT max(a - b, 0), ADD min(a + b, 255), ABSDIFF |a - b|, MIN, MAX
 *                   (cv2.subtract, cv2.add, cv2.absdiff, cv2.min, cv2.max on uint8)
 *   VF_STEP_MIX     cv2.transform: `data` is the 12 int32 [M | t] of vf_mix_*, with `shift`, and
 *                   `op` a VF_ROUND_*; 3-channel frames only
 *   VF_STEP_SEP     the separable filter: `data` is 1 + kw + kh int32, the divisor (0 or 1: none),
 *                   then kx, then ky; `kw`, `kh` the tap counts, `shift`, `op` a VF_ROUND_*, `border`
 *   VF_STEP_LEVEL   the level filter: `op` a VF_LEVEL_*, `data` 4 int32 {mask, link, clip_lo, clip_hi}.
 *                   It reads its whole operand, so a program that holds one runs on whole frames
 *                   only: vf_chain_frames_host refuses a frame that does not fit the staging whole
 *   VF_STEP_CLAHE   CLAHE: `data` 4 int32 {mask, clip_q8, tiles_x, tiles_y}.  It reads its whole
 *                   operand as well, with the same refusal
 *   VF_STEP_WARP    the affine warp: `data` six float64 m, then six int32 {mode, interp, value B,
 *                   G, R, 0} (48 + 24 bytes), with `border`.  It reads anywhere in its operand: the
 *                   same refusal, and it never runs in place
 *   VF_STEP_RESIZE  the resize: `data` two float64 {fx, fy}, then four int32 {dw, dh, interp, 0}
 *                   (16 + 16 bytes).  Its value has another size than its operand; every other
 *                   step makes a value of its operand's size, and a binary step whose operands
 *                   differ in size is refused per frame, naming the step.  The same refusal of a
 *                   frame, or of any value, that does not fit the staging whole; never in place
 * `data` is a HOST pointer, read during the call only.  VF_E_INVALID, before any GPU work: a step
 * that reads a later value or itself, a value other than the last that no step reads, a 3-channel
 * table or a colour matrix on 1-channel frames, more than VF_CHAIN_MAX_STEPS steps, and anything
 * the single-filter entry points refuse for a table, a kernel, an element or a matrix.
 * The VF_STEP_* values are not dense: 4 names no kind and stays refused ("unknown kind 4"), as
 * callers' checks of the refusal expect, so VF_STEP_MIX is 5; 6 likewise, so VF_STEP_SEP is 7 and
 * VF_STEP_LEVEL 8; 9 stays refused too, so VF_STEP_CLAHE is 10; 11 stays refused, so
 * VF_STEP_WARP is 12; 13 stays refused, so VF_STEP_RESIZE is 14, and 15 stays refused. */
#define VF_STEP_TABLE  0
#define VF_STEP_CONV   1
#define VF_STEP_RANK   2
#define VF_STEP_BINARY 3
#define VF_STEP_MIX    5
#define VF_STEP_SEP    7
#define VF_STEP_LEVEL  8
#define VF_STEP_CLAHE  10
#define VF_STEP_WARP   12
#define VF_STEP_RESIZE 14
#define VF_BIN_SUBTRACT 0
#define VF_BIN_ADD      1
#define VF_BIN_ABSDIFF  2
#define VF_BIN_MIN      3
#define VF_BIN_MAX      4
#define VF_CHAIN_MAX_STEPS 8

typedef struct vf_step {
  int kind;         /* a VF_STEP_* */
  int a, b;         /* operand values; b for VF_STEP_BINARY only */
  int op;           /* VF_STEP_RANK: a VF_RANK_*; VF_STEP_BINARY: a VF_BIN_*; VF_STEP_MIX, VF_STEP_SEP: a VF_ROUND_*; VF_STEP_LEVEL: a VF_LEVEL_* */
  const void *data; /* the table, the int16 weights, the element or the int32 of a matrix, of
                       separable taps, of a level step or of a CLAHE step, or a warp or resize
                       step's doubles and int32 (host memory) */
  int kw, kh;       /* VF_STEP_CONV, VF_STEP_RANK, VF_STEP_SEP */
  int shift;        /* VF_STEP_CONV, VF_STEP_MIX, VF_STEP_SEP */
  int border;       /* VF_STEP_CONV, VF_STEP_RANK, VF_STEP_SEP, VF_STEP_WARP: a VF_BORDER_* */
  int channels;     /* VF_STEP_TABLE: 1 or 3 */
} vf_step;

/* Enqueue ddst[i] = op(da[i], db[i]) over nbytes of device memory on `stream`, op a VF_BIN_*.
 * Returns after the launch (does not synchronise); each pointer at any alignment.  ddst == da or
 * ddst == db exactly is allowed; a partial overlap of ddst with either, a NULL pointer or an
 * unknown op is VF_E_INVALID.  nbytes == 0 is VF_OK and writes nothing. */
int vf_binary_device(vf_ctx *ctx, const void *da, const void *db, void *ddst, size_t nbytes,
                     int op, void *stream);

/* The program on `n` separately allocated host frames (srcs[i] -> dsts[i], widths[i] x heights[i]
 * x channels), synchronous, as vf_conv_frames_host: srcs[i] == dsts[i] is allowed; a frame larger
 * than the context's staging is cut into bands of rows with the program's total vertical reach R
 * (the largest summed radius along a path) as halo; VF_E_INVALID when 2 R + 1 rows of a frame do
 * not fit it.  Intermediate values live in device scratch of the context, allocated by the first
 * call that needs them and freed with the context.  dsts[i] holds frame i's RESULT, whose size is
 * the frame's unless the program holds a resize step (the function below says it); then srcs[i]
 * and dsts[i] may be equal or overlap only where the two sizes are equal. */
int vf_chain_frames_host(vf_ctx *ctx, const uint8_t *const *srcs, uint8_t *const *dsts,
                         const int *widths, const int *heights, int n, int channels,
                         const vf_step *steps, int nsteps);

/* The size of the program's result for a frame of width x height, with every check that
 * vf_chain_frames_host makes of the steps and of the sizes of the values.  No GPU work. */
int vf_chain_out_size(vf_ctx *ctx, const vf_step *steps, int nsteps, int channels, int width,
                      int height, int *out_w, int *out_h);

/* vf_jpeg_invert with the program in place of the inversion: decode -> the steps -> encode on
 * the GPU with one decode and one encode, on the decoded BGR frame (3 channels).  A program that
 * folds to a single table runs in the fused colour stage, as vf_jpeg_lut does.  A program with a
 * resize step is encoded at its result's size, frame by frame. */
int vf_jpeg_chain(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                  const vf_step *steps, int nsteps, int quality, int subsamp, int flags,
                  uint8_t *const *outs, const size_t *caps, size_t *sizes);

/* vf_jpeg_invert_submit with the program (copied, with every table, kernel and element: the
 * caller may reuse them at once).  The ticket is an invert ticket: collect with
 * vf_jpeg_invert_query / _wait / _fetch / _scatter. */
int vf_jpeg_chain_submit(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                         const vf_step *steps, int nsteps, int quality, int subsamp, int flags,
                         uint64_t *ticket);

/* vf_jpeg_bench_invert with the program between the decode and the encode. */
int vf_jpeg_bench_chain(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                        const vf_step *steps, int nsteps, int quality, int subsamp, int flags,
                        int iters, float *ms, float *stage_ms);

#ifdef __cplusplus
}
#endif

#endif /* VFILTER_H */
