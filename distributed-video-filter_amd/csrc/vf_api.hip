// vf_api.hip — C ABI of libvfilter_hip.so (declared in include/vfilter.h).
//
// Host side of the MI355X frame filter.  What it replaces in the reference:
//   * InverterWorker per-process state          inverter.py:10-20   -> vf_create / vf_destroy
//   * cv2.bitwise_not(frame) on one frame       inverter.py:41      -> vf_invert_host
//   * the one-frame-per-iteration worker loop   worker.py:35-57     -> vf_invert_batch_host,
//                                                                      vf_invert_frames_host,
//                                                                      vf_invert_frames_async
// Every host->host call becomes a job of the context's Engine (vf_engine.hip): a thread that
// streams the job's bytes through a ring of device slots (H2D on one SDMA engine, the invert
// kernel, D2H on the other) without draining between jobs.  Synchronous entry points submit
// and wait; the asynchronous one returns a ticket.  Pageable caller memory is staged through
// pinned slot buffers by a host copy pool; page-locked caller memory (vf_alloc_host,
// vf_host_register — e.g. a shared-memory frame ring) is DMA'd directly with no host copy.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/vfilter.h"
#include "vf_env.h"
#include "vf_host_mem.h"
#include "vf_internal.h"
#include "vf_sep_plan.h"
#include "vf_level_plan.h"
#include "vf_clahe_plan.h"
#include "vf_resize_plan.h"
#include "vf_warp_plan.h"
#include "vf_jpeg_codec.h"
#include "vf_lut_split.h"
#include "vf_conv_bands.h"
#include "vf_tile_plan.h"
#include "vf_chain_plan.h"

#define VF_EXPORT extern "C" __attribute__((visibility("default")))

namespace {

constexpr int kMaxSlots = 8;

struct ErrState {
  int hip = 0;
  char msg[512] = "no error";
};
thread_local ErrState g_thread_err;

using vf::env_size;

}  // namespace

struct vf_ctx {
  int device = -1;
  int num_cus = 256;
  vf::LaunchCfg cfg;
  vf::Engine *engine = nullptr;
  int hip = 0;
  char msg[512] = "no error";
  std::mutex err_mu;  // msg / hip: JPEG calls on one context may fail on two threads at once
  // results of the last host->host job waited on (vf_elapsed_ms / vf_last_timeline)
  float last_kernel_ms = 0.f;
  std::vector<vf::ChunkTime> timeline;
  // JPEG codecs (created on first use, at most VF_JPEG_CODECS, default 2): each has its own
  // stream and buffers, so JPEG calls from two host threads overlap one batch's host work
  // (parse, staging, copy-out) with the other's GPU work.
  std::mutex jpeg_mu;
  std::condition_variable jpeg_cv;
  std::vector<vf::jpeg::Codec *> jpeg_all, jpeg_free;
  vf::jpeg::ComputeGate jpeg_gate;
  // submitted vf_jpeg_invert_submit batches: ticket -> the codec that holds it until fetched
  std::map<uint64_t, vf::jpeg::Codec *> jpeg_jobs;
  uint64_t jpeg_next_ticket = 1;
  // decoder frame-size limit (vf_jpeg_set_max_pixels), applied to a codec whenever it is leased
  std::atomic<uint64_t> jpeg_max_pixels{vf::jpeg::kDefaultMaxPixels};
  // vf_bench_device_ring's region events, created once (not inside a caller's timed region)
  hipEvent_t bench_ev[2] = {nullptr, nullptr};
  // the raw host path's staging, shared by vf_lut_frames_host and vf_conv_frames_host: a stream and
  // one input and one output device buffer of raw_cap (+ slack) bytes, created by the first call of
  // either; raw_cap is the engine's slot size
  std::mutex raw_mu;
  size_t raw_cap = 0;
  hipStream_t raw_stream = nullptr;
  uint8_t *raw_din = nullptr, *raw_dout = nullptr;
  // program_frames_host's intermediate values: device buffers sized like raw_din, allocated by the
  // first program that needs them (raw_mu held; one of a single step needs none), freed with the context
  std::vector<uint8_t *> raw_scratch;
  // the level filter's histogram words (vf_level.hip): level_hist for program_frames_host and
  // vf_hist_frames_host (raw_mu held, raw_stream), level::kHistWords for each step of a program;
  // level_dev_hist for vf_level_device (level_mu guards its creation; the caller's stream orders its use)
  uint32_t *level_hist = nullptr;
  std::mutex level_mu;
  uint32_t *level_dev_hist = nullptr;
  // the same for a program with CLAHE steps (vf_clahe.hip): level_hist then holds
  // chain::whole_frame_scratch_bytes of the program, level_hist_bytes what it holds now; clahe_dev
  // is vf_clahe_device's clahe::kScratchBytes (level_mu guards its creation)
  size_t level_hist_bytes = 0;
  void *clahe_dev = nullptr;
};

namespace {

int set_err(vf_ctx *ctx, int status, int hip, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  ErrState &t = g_thread_err;
  t.hip = hip;
  std::snprintf(t.msg, sizeof t.msg, "%s", buf);
  if (ctx) {
    std::lock_guard<std::mutex> lk(ctx->err_mu);
    ctx->hip = hip;
    std::snprintf(ctx->msg, sizeof ctx->msg, "%s", buf);
  }
  return status;
}

int fail_hip(vf_ctx *ctx, hipError_t e, const char *what, int line) {
  return set_err(ctx, VF_E_HIP, (int)e, "%s failed: %s (%s, vf_api.hip:%d)", what,
                 hipGetErrorString(e), hipGetErrorName(e), line);
}

#define VF_HIP(ctx, call)                                              \
  do {                                                                 \
    hipError_t e_ = (call);                                            \
    if (e_ != hipSuccess) return fail_hip((ctx), e_, #call, __LINE__); \
  } while (0)

#define VF_CHECK_CTX(ctx)                                                             \
  do {                                                                                \
    if (!(ctx)) return set_err(nullptr, VF_E_INVALID, 0, "%s: ctx is NULL", __func__); \
  } while (0)

bool overlaps_partially(const uint8_t *a, const uint8_t *b, size_t n) {
  if (a == b || n == 0) return false;
  return (a < b + n) && (b < a + n);
}

// Wait for a job and publish its result on the context.
int finish(vf_ctx *ctx, uint64_t id, float *gpu_ms) {
  vf::JobResult r;
  if (!ctx->engine->wait(id, &r))
    return set_err(ctx, VF_E_INVALID, 0, "vf_wait: unknown ticket %llu", (unsigned long long)id);
  if (gpu_ms) *gpu_ms = r.gpu_ms;
  ctx->last_kernel_ms = r.kernel_ms;
  ctx->timeline = std::move(r.timeline);
  if (r.status != VF_OK) return set_err(ctx, r.status, (int)r.hip, "%s", r.msg.c_str());
  return VF_OK;
}

// Validate a frame list into engine segments (empty frames dropped).
int frames_to_segs(vf_ctx *ctx, const char *fn, const uint8_t *const *srcs, uint8_t *const *dsts,
                   const size_t *nbytes, int n, std::vector<vf::Seg> *segs) {
  if (n < 0) return set_err(ctx, VF_E_INVALID, 0, "%s: n < 0", fn);
  if (n > 0 && (!srcs || !dsts || !nbytes)) return set_err(ctx, VF_E_INVALID, 0, "%s: NULL array", fn);
  segs->reserve((size_t)n);
  for (int i = 0; i < n; ++i) {
    if (nbytes[i] == 0) continue;
    if (!srcs[i] || !dsts[i]) return set_err(ctx, VF_E_INVALID, 0, "%s: frame %d has a NULL buffer", fn, i);
    if (overlaps_partially(srcs[i], dsts[i], nbytes[i]))
      return set_err(ctx, VF_E_INVALID, 0, "%s: frame %d src/dst partially overlap", fn, i);
    segs->push_back(vf::Seg{srcs[i], dsts[i], nbytes[i]});
  }
  return VF_OK;
}

int run_sync(vf_ctx *ctx, std::vector<vf::Seg> &&segs) {
  if (segs.empty()) {
    ctx->last_kernel_ms = 0.f;
    ctx->timeline.clear();
    return VF_OK;
  }
  vf::JobResult r;
  if (ctx->engine->run_now(segs, &r)) {  // page-locked, device-mapped: launched from this thread
    ctx->last_kernel_ms = r.kernel_ms;
    ctx->timeline = std::move(r.timeline);
    if (r.status != VF_OK) return set_err(ctx, r.status, (int)r.hip, "%s", r.msg.c_str());
    return VF_OK;
  }
  return finish(ctx, ctx->engine->submit(std::move(segs)), nullptr);
}

}  // namespace

// ---- library / context ---------------------------------------------------------------

VF_EXPORT int vf_get_abi_version(void) { return VF_ABI_VERSION; }

VF_EXPORT const char *vf_status_string(int status) {
  switch (status) {
    case VF_OK: return "VF_OK";
    case VF_E_INVALID: return "VF_E_INVALID: invalid argument";
    case VF_E_HIP: return "VF_E_HIP: HIP runtime error";
    case VF_E_NOMEM: return "VF_E_NOMEM: out of memory";
    case VF_E_NODEVICE: return "VF_E_NODEVICE: no usable gfx950 device";
    case VF_E_JPEG: return "VF_E_JPEG: malformed or unsupported JPEG";
    default: return "unknown vfilter status";
  }
}

VF_EXPORT int vf_device_count(int *out_count) {
  if (!out_count) return set_err(nullptr, VF_E_INVALID, 0, "vf_device_count: out_count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    n = 0;
  }
  *out_count = n;
  return VF_OK;
}

VF_EXPORT int vf_device_pci_bus_id(int device, char *buf, int len) {
  if (!buf || len < 13) return set_err(nullptr, VF_E_INVALID, 0, "vf_device_pci_bus_id: buffer too small");
  buf[0] = 0;
  int ndev = 0;
  vf_device_count(&ndev);
  if (device < 0 || device >= ndev)
    return set_err(nullptr, VF_E_NODEVICE, 0, "vf_device_pci_bus_id: device %d not available (%d visible)",
                   device, ndev);
  hipError_t e = hipDeviceGetPCIBusId(buf, len, device);
  if (e != hipSuccess) return fail_hip(nullptr, e, "hipDeviceGetPCIBusId", __LINE__);
  return VF_OK;
}

VF_EXPORT int vf_create(int device, size_t max_frame_bytes, int max_batch, vf_ctx **out) {
  if (!out) return set_err(nullptr, VF_E_INVALID, 0, "vf_create: out is NULL");
  *out = nullptr;
  if (max_batch < 1) max_batch = 1;
  int ndev = 0;
  vf_device_count(&ndev);
  if (device < 0 || device >= ndev)
    return set_err(nullptr, VF_E_NODEVICE, 0, "vf_create: device %d not available (%d visible)",
                   device, ndev);
  hipDeviceProp_t prop;
  hipError_t e = hipGetDeviceProperties(&prop, device);
  if (e != hipSuccess) return fail_hip(nullptr, e, "hipGetDeviceProperties", __LINE__);
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return set_err(nullptr, VF_E_NODEVICE, 0,
                   "vf_create: device %d is %s; libvfilter_hip.so is built for gfx950 only",
                   device, prop.gcnArchName);
  vf_ctx *ctx = new (std::nothrow) vf_ctx();
  if (!ctx) return set_err(nullptr, VF_E_NOMEM, 0, "vf_create: out of host memory");
  ctx->device = device;
  ctx->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  ctx->cfg.max_blocks = (int)env_size("VF_MAX_BLOCKS", (size_t)ctx->num_cus * 32);
  if (ctx->cfg.max_blocks < 1) ctx->cfg.max_blocks = ctx->num_cus * 32;
  const int nslots = (int)std::min<size_t>(kMaxSlots, std::max<size_t>(2, env_size("VF_SLOTS", 4)));
  size_t want = max_frame_bytes ? max_frame_bytes * (size_t)max_batch : (size_t)8 << 20;
  size_t slot = env_size("VF_SLOT_BYTES", std::min(want, (size_t)16 << 20));
  slot = std::max<size_t>(slot, (size_t)1 << 20);
  slot = std::min<size_t>(slot, (size_t)64 << 20);
  slot = (slot + 4095) & ~(size_t)4095;
  ctx->engine = new (std::nothrow) vf::Engine();
  std::string err;
  e = ctx->engine ? ctx->engine->init(device, nslots, slot, ctx->cfg, &err) : hipErrorOutOfMemory;
  if (e != hipSuccess) {
    int st = (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) ? VF_E_NOMEM : VF_E_HIP;
    set_err(nullptr, st, (int)e, "vf_create: %s", err.empty() ? hipGetErrorString(e) : err.c_str());
    delete ctx->engine;
    delete ctx;
    return st;
  }
  ctx->raw_cap = slot;
  *out = ctx;
  return VF_OK;
}

VF_EXPORT int vf_destroy(vf_ctx *ctx) {
  if (!ctx) return VF_OK;
  if (ctx->raw_stream) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->raw_stream);
    (void)hipFree(ctx->raw_din);
    (void)hipFree(ctx->raw_dout);
    for (uint8_t *p : ctx->raw_scratch) (void)hipFree(p);
    if (ctx->level_hist) (void)hipFree(ctx->level_hist);
    if (ctx->level_dev_hist) (void)hipFree(ctx->level_dev_hist);
    if (ctx->clahe_dev) (void)hipFree(ctx->clahe_dev);
    (void)hipStreamDestroy(ctx->raw_stream);
  }
  for (vf::jpeg::Codec *c : ctx->jpeg_all) delete c;  // each synchronises its stream first
  delete ctx->engine;  // finishes queued jobs first
  for (hipEvent_t e : ctx->bench_ev)
    if (e) (void)hipEventDestroy(e);
  delete ctx;
  return VF_OK;
}

VF_EXPORT const char *vf_last_error(const vf_ctx *ctx) { return ctx ? ctx->msg : g_thread_err.msg; }

VF_EXPORT int vf_last_hip_error(const vf_ctx *ctx) { return ctx ? ctx->hip : g_thread_err.hip; }

VF_EXPORT int vf_ctx_device(const vf_ctx *ctx, int *out_device) {
  if (!ctx || !out_device) return set_err(nullptr, VF_E_INVALID, 0, "vf_ctx_device: NULL argument");
  *out_device = ctx->device;
  return VF_OK;
}

// ---- host -> host ----------------------------------------------------------------------

VF_EXPORT int vf_invert_host(vf_ctx *ctx, const uint8_t *src, uint8_t *dst, size_t nbytes) {
  VF_CHECK_CTX(ctx);
  if (nbytes && (!src || !dst)) return set_err(ctx, VF_E_INVALID, 0, "vf_invert_host: NULL buffer");
  if (overlaps_partially(src, dst, nbytes))
    return set_err(ctx, VF_E_INVALID, 0, "vf_invert_host: src and dst partially overlap");
  std::vector<vf::Seg> segs;
  if (nbytes) segs.push_back(vf::Seg{src, dst, nbytes});
  return run_sync(ctx, std::move(segs));
}

VF_EXPORT int vf_invert_batch_host(vf_ctx *ctx, const uint8_t *src, uint8_t *dst,
                                   size_t frame_bytes, int n) {
  VF_CHECK_CTX(ctx);
  if (n < 0) return set_err(ctx, VF_E_INVALID, 0, "vf_invert_batch_host: n < 0");
  if (n && frame_bytes > SIZE_MAX / (size_t)n)
    return set_err(ctx, VF_E_INVALID, 0, "vf_invert_batch_host: size overflow");
  return vf_invert_host(ctx, src, dst, frame_bytes * (size_t)n);
}

VF_EXPORT int vf_invert_frames_host(vf_ctx *ctx, const uint8_t *const *srcs, uint8_t *const *dsts,
                                    const size_t *nbytes, int n) {
  VF_CHECK_CTX(ctx);
  std::vector<vf::Seg> segs;
  int rc = frames_to_segs(ctx, "vf_invert_frames_host", srcs, dsts, nbytes, n, &segs);
  return rc != VF_OK ? rc : run_sync(ctx, std::move(segs));
}

VF_EXPORT int vf_invert_frames_async(vf_ctx *ctx, const uint8_t *const *srcs, uint8_t *const *dsts,
                                     const size_t *nbytes, int n, uint64_t *ticket) {
  VF_CHECK_CTX(ctx);
  if (!ticket) return set_err(ctx, VF_E_INVALID, 0, "vf_invert_frames_async: ticket is NULL");
  *ticket = 0;
  std::vector<vf::Seg> segs;
  int rc = frames_to_segs(ctx, "vf_invert_frames_async", srcs, dsts, nbytes, n, &segs);
  if (rc != VF_OK) return rc;
  *ticket = ctx->engine->submit(std::move(segs));
  return VF_OK;
}

VF_EXPORT int vf_wait(vf_ctx *ctx, uint64_t ticket, float *gpu_ms) {
  VF_CHECK_CTX(ctx);
  if (gpu_ms) *gpu_ms = -1.f;
  return finish(ctx, ticket, gpu_ms);
}

VF_EXPORT int vf_query(vf_ctx *ctx, uint64_t ticket, int *done) {
  VF_CHECK_CTX(ctx);
  if (!done) return set_err(ctx, VF_E_INVALID, 0, "vf_query: done is NULL");
  bool d = false;
  if (!ctx->engine->query(ticket, &d))
    return set_err(ctx, VF_E_INVALID, 0, "vf_query: unknown ticket %llu", (unsigned long long)ticket);
  *done = d ? 1 : 0;
  return VF_OK;
}

// ---- device-resident ---------------------------------------------------------------------

VF_EXPORT int vf_invert_device(vf_ctx *ctx, const void *dsrc, void *ddst, size_t nbytes,
                               void *stream) {
  VF_CHECK_CTX(ctx);
  if (nbytes == 0) return VF_OK;
  if (!dsrc || !ddst) return set_err(ctx, VF_E_INVALID, 0, "vf_invert_device: NULL buffer");
  if (overlaps_partially((const uint8_t *)dsrc, (const uint8_t *)ddst, nbytes))
    return set_err(ctx, VF_E_INVALID, 0, "vf_invert_device: src and dst partially overlap");
  VF_HIP(ctx, hipSetDevice(ctx->device));
  VF_HIP(ctx, vf::launch_invert(dsrc, ddst, nbytes, ctx->cfg, (hipStream_t)stream));
  return VF_OK;
}

VF_EXPORT int vf_invert_device_frames(vf_ctx *ctx, const void *const *dsrcs, void *const *ddsts,
                                      const size_t *nbytes, int n, size_t total_bytes,
                                      void *stream) {
  VF_CHECK_CTX(ctx);
  if (n < 0 || n > 65535)
    return set_err(ctx, VF_E_INVALID, 0, "vf_invert_device_frames: n=%d outside [0, 65535]", n);
  if (n == 0) return VF_OK;
  if (!dsrcs || !ddsts || !nbytes)
    return set_err(ctx, VF_E_INVALID, 0, "vf_invert_device_frames: NULL descriptor array");
  VF_HIP(ctx, hipSetDevice(ctx->device));
  VF_HIP(ctx, vf::launch_invert_frames(dsrcs, ddsts, nbytes, n, total_bytes, ctx->cfg,
                                       (hipStream_t)stream));
  return VF_OK;
}

// ---- 256-entry table filter (cv2.LUT) on raw frames ------------------------------------------

namespace {

int check_table(vf_ctx *ctx, const char *fn, const uint8_t *table, int channels) {
  if (!table) return set_err(ctx, VF_E_INVALID, 0, "%s: table is NULL", fn);
  if (channels != 1 && channels != 3)
    return set_err(ctx, VF_E_INVALID, 0, "%s: channels=%d, a table has 1 or 3", fn, channels);
  return VF_OK;
}

// The raw host path's stream and device buffers (ctx->raw_mu held); fn: the entry point that asks.
int raw_staging(vf_ctx *ctx, const char *fn, size_t alloc) {
  if (ctx->raw_stream) return VF_OK;
  hipStream_t st = nullptr;
  VF_HIP(ctx, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  void *din = nullptr, *dout = nullptr;
  hipError_t e = hipMalloc(&din, alloc);
  if (e == hipSuccess) e = hipMalloc(&dout, alloc);
  if (e != hipSuccess) {
    (void)hipFree(din);
    (void)hipStreamDestroy(st);
    return set_err(ctx, VF_E_NOMEM, (int)e, "%s: hipMalloc(%zu) failed: %s", fn, alloc, hipGetErrorString(e));
  }
  ctx->raw_din = static_cast<uint8_t *>(din);
  ctx->raw_dout = static_cast<uint8_t *>(dout);
  ctx->raw_stream = st;
  return VF_OK;
}

}  // namespace

VF_EXPORT int vf_lut_device(vf_ctx *ctx, const void *dsrc, void *ddst, size_t nbytes, const uint8_t *table,
                            int channels, void *stream) {
  VF_CHECK_CTX(ctx);
  int rc = check_table(ctx, "vf_lut_device", table, channels);
  if (rc != VF_OK) return rc;
  if (channels == 3 && nbytes % 3 != 0)
    return set_err(ctx, VF_E_INVALID, 0, "vf_lut_device: %zu bytes are not whole 3-channel pixels", nbytes);
  if (nbytes == 0) return VF_OK;
  if (!dsrc || !ddst) return set_err(ctx, VF_E_INVALID, 0, "vf_lut_device: NULL buffer");
  if (overlaps_partially((const uint8_t *)dsrc, (const uint8_t *)ddst, nbytes))
    return set_err(ctx, VF_E_INVALID, 0, "vf_lut_device: src and dst partially overlap");
  VF_HIP(ctx, hipSetDevice(ctx->device));
  VF_HIP(ctx, vf::launch_lut(dsrc, ddst, nbytes, table, channels, 0, ctx->cfg, (hipStream_t)stream));
  return VF_OK;
}

VF_EXPORT int vf_lut_frames_host(vf_ctx *ctx, const uint8_t *const *srcs, uint8_t *const *dsts, const size_t *nbytes,
                                 int n, const uint8_t *table, int channels) {
  VF_CHECK_CTX(ctx);
  int rc = check_table(ctx, "vf_lut_frames_host", table, channels);
  if (rc != VF_OK) return rc;
  std::vector<vf::Seg> segs;
  if ((rc = frames_to_segs(ctx, "vf_lut_frames_host", srcs, dsts, nbytes, n, &segs)) != VF_OK) return rc;
  std::vector<vf::lut::Frame> frames;
  frames.reserve(segs.size());
  for (const vf::Seg &sg : segs) {
    if (channels == 3 && sg.len % 3 != 0)
      return set_err(ctx, VF_E_INVALID, 0, "vf_lut_frames_host: a frame of %zu bytes is not whole 3-channel pixels",
                     sg.len);
    frames.push_back(vf::lut::Frame{sg.src, sg.dst, sg.len});
  }
  if (frames.empty()) return VF_OK;
  std::lock_guard<std::mutex> lk(ctx->raw_mu);
  VF_HIP(ctx, hipSetDevice(ctx->device));
  // a piece sits in both device buffers at its caller pointers' offsets mod 16 past a 16-B
  // boundary, so the copies and the kernel see the caller's alignment: up to 15 bytes of slack
  const size_t cap = ctx->raw_cap, alloc = ((cap + 15 + 15) & ~(size_t)15);
  if ((rc = raw_staging(ctx, "vf_lut_frames_host", alloc)) != VF_OK) return rc;
  const std::vector<vf::lut::Launch> ls = vf::lut::split(frames, cap, channels);
  hipStream_t st = ctx->raw_stream;
  std::vector<size_t> at(ls.size());
  for (size_t i = 0; i < ls.size();) {
    // one fill of the buffers: upload and filter the pieces that fit, download them, wait
    size_t cur = 0, j = i;
    for (; j < ls.size(); ++j) {
      const size_t room = (ls[j].len + 15 + 15) & ~(size_t)15;
      if (cur + room > alloc) break;
      const uint8_t *din = ctx->raw_din + cur + ((uintptr_t)ls[j].src & 15);
      uint8_t *dout = ctx->raw_dout + cur + ((uintptr_t)ls[j].dst & 15);
      at[j] = cur;
      cur += room;
      VF_HIP(ctx, hipMemcpyAsync(const_cast<uint8_t *>(din), ls[j].src, ls[j].len, hipMemcpyHostToDevice, st));
      VF_HIP(ctx, vf::launch_lut(din, dout, ls[j].len, table, channels, ls[j].phase, ctx->cfg, st));
    }
    for (size_t k = i; k < j; ++k)
      VF_HIP(ctx, hipMemcpyAsync(ls[k].dst, ctx->raw_dout + at[k] + ((uintptr_t)ls[k].dst & 15), ls[k].len,
                                 hipMemcpyDeviceToHost, st));
    VF_HIP(ctx, hipStreamSynchronize(st));
    i = j;
  }
  return VF_OK;
}

// ---- 2-D convolution filter (cv2.filter2D) on raw frames ---------------------------------------

namespace {

// The kernel arguments every vf_conv_* / vf_jpeg_conv* entry point shares.
int check_kernel(vf_ctx *ctx, const char *fn, const int16_t *weights, int kw, int kh, int shift, int border) {
  if (!weights) return set_err(ctx, VF_E_INVALID, 0, "%s: weights is NULL", fn);
  if (!vf::tile::sides_ok(kw, kh))
    return set_err(ctx, VF_E_INVALID, 0, "%s: a %d x %d kernel; sides are odd and at most %d", fn, kw, kh,
                   vf::conv::kMaxK);
  if (shift < 0 || shift > 16) return set_err(ctx, VF_E_INVALID, 0, "%s: shift=%d outside 0..16", fn, shift);
  long sum = 0;
  for (int i = 0; i < kw * kh; ++i) sum += std::labs((long)weights[i]);
  if (sum > 65536) return set_err(ctx, VF_E_INVALID, 0, "%s: sum|K| = %ld exceeds 65536", fn, sum);
  if (!vf::tile::border_ok(border)) return set_err(ctx, VF_E_INVALID, 0, "%s: unknown border %d", fn, border);
  return VF_OK;
}

int check_frame_shape(vf_ctx *ctx, const char *fn, int width, int height, int channels) {
  if (width <= 0 || height <= 0)
    return set_err(ctx, VF_E_INVALID, 0, "%s: a %d x %d frame", fn, width, height);
  if ((uint64_t)width * (uint64_t)channels > 0x7FFFFFFFull)
    return set_err(ctx, VF_E_INVALID, 0, "%s: rows of %d pixels are too long", fn, width);
  return VF_OK;
}

int check_channels(vf_ctx *ctx, const char *fn, int channels) {
  if (channels != 1 && channels != 3)
    return set_err(ctx, VF_E_INVALID, 0, "%s: channels=%d, a frame has 1 or 3", fn, channels);
  return VF_OK;
}

// The frame arguments vf_conv_device and vf_rank_device share; 1 for the empty frame: nothing to do.
int check_device_frame(vf_ctx *ctx, const char *fn, const void *dsrc, const void *ddst, int width, int height,
                       int channels) {
  int rc = check_channels(ctx, fn, channels);
  if (rc != VF_OK) return rc;
  if (width == 0 && height == 0) return 1;
  if ((rc = check_frame_shape(ctx, fn, width, height, channels)) != VF_OK) return rc;
  if (!dsrc || !ddst) return set_err(ctx, VF_E_INVALID, 0, "%s: NULL buffer", fn);
  const size_t nbytes = (size_t)width * (size_t)channels * (size_t)height;
  const uint8_t *s = (const uint8_t *)dsrc, *d = (const uint8_t *)ddst;
  if (s < d + nbytes && d < s + nbytes)  // out of place only: a tap reads what a neighbour writes
    return set_err(ctx, VF_E_INVALID, 0, "%s: src and dst overlap", fn);
  return VF_OK;
}

}  // namespace

VF_EXPORT int vf_conv_device(vf_ctx *ctx, const void *dsrc, void *ddst, int width, int height, int channels,
                             const int16_t *weights, int kw, int kh, int shift, int border, void *stream) {
  VF_CHECK_CTX(ctx);
  int rc = check_kernel(ctx, "vf_conv_device", weights, kw, kh, shift, border);
  if (rc != VF_OK) return rc;
  if ((rc = check_device_frame(ctx, "vf_conv_device", dsrc, ddst, width, height, channels)) != VF_OK)
    return rc < 0 ? rc : VF_OK;
  VF_HIP(ctx, hipSetDevice(ctx->device));
  VF_HIP(ctx, vf::launch_conv(dsrc, ddst, width, channels, height, 0, height, 0, height, weights, kw, kh, shift, border,
                              vf::conv_form_env(), (hipStream_t)stream));
  return VF_OK;
}

// ---- programs: every chain, and a convolution or rank filter as a program of one step ------------

// The one place that turns the steps of a program into kernel launches (declared in vf_internal.h):
// it walks vf_chain_plan.h's band_launches and switches on the step's kind.  The raw host path
// below and the JPEG path (vf_jpeg_host.hip) both come here; neither launches a step's kernel itself.
namespace vf {

hipError_t run_launches(const chain::Program &prog, const uint64_t *masks, const std::vector<chain::Launch> &launches,
                        uint8_t *const *bufs, uint8_t *out, int w, int channels, int frame_h, int conv_form,
                        uint32_t *hist, const LaunchCfg &cfg, hipStream_t stream) {
  const int frame_w = w, frame_rows = frame_h;
  for (const chain::Launch &l : launches) {
    const chain::Step &s = prog.steps[(size_t)l.step - 1];
    // a program with a resize step (chain::frame_launches): every value has a size of its own, and
    // the launch says its operand's, which is the result's too for every step but the resize
    if (l.a_w) w = l.a_w, frame_h = l.a_h;
    else w = frame_w, frame_h = frame_rows;
    // `row` is the OPERAND's pitch.  It addresses dst as well because every step but the resize makes a value of
    // its operand's size, and a resize launch comes from frame_launches, whose row offsets are all 0 (dst_row * row
    // is 0 whatever the pitch) and whose kernel takes the result's size from the step, not from nbytes.
    const size_t row = (size_t)w * (size_t)channels;
    const uint8_t *a = bufs[l.a_buf] + (size_t)l.a_row * row;
    uint8_t *dst = l.dst_buf == chain::kOut ? out : bufs[l.dst_buf] + (size_t)l.dst_row * row;
    const size_t nbytes = (size_t)l.nrows * row;
    hipError_t e;
    if (s.kind == chain::kTable)
      e = launch_lut(a, dst, nbytes, s.table.data(), s.channels, 0, cfg, stream);
    else if (s.kind == chain::kBinary)
      e = launch_binary(a, bufs[l.b_buf] + (size_t)l.b_row * row, dst, nbytes, s.op, cfg, stream);
    else if (s.kind == chain::kConv)
      e = launch_conv(a, dst, w, channels, frame_h, l.y0, l.nrows, l.src0, l.nsrc, s.weights.data(), s.kw, s.kh,
                      s.shift, s.border, conv_form, stream);
    else if (s.kind == chain::kRank)
      e = launch_rank(a, dst, w, channels, frame_h, l.y0, l.nrows, l.src0, l.nsrc, s.op, masks[l.step - 1], s.kw, s.kh,
                      s.border, stream);
    else if (s.kind == chain::kMix)
      e = launch_mix(a, dst, nbytes, s.matrix.data(), s.shift, s.op, cfg, stream);
    else if (s.kind == chain::kSep)
      e = launch_sep(a, dst, w, channels, frame_h, l.y0, l.nrows, l.src0, l.nsrc, s.taps_x.data(), s.kw, s.taps_y.data(),
                     s.kh, s.shift, s.divisor, s.op, s.border, sep_form_env(), stream);
    else if (s.kind == chain::kLevel)  // whole frames only (chain::whole_frame): nbytes is all of the operand
      e = hist ? launch_level(a, dst, nbytes, channels, s.op, s.mask, s.link, s.clip_lo, s.clip_hi,
                              hist + (size_t)(l.step - 1) * level::kHistWords, cfg, stream)
               : hipErrorInvalidValue;
    else if (s.kind == chain::kClahe)  // whole frames only as well: the operand is frame_h rows
      e = hist && l.nrows == frame_h
              ? launch_clahe(a, dst, w, frame_h, channels, s.clip_q8, s.tiles_x, s.tiles_y, s.mask,
                             reinterpret_cast<uint8_t *>(hist) + chain::level_scratch_bytes() +
                                 (size_t)chain::clahe_steps_before(prog, l.step) * clahe::kScratchBytes,
                             stream)
              : hipErrorInvalidValue;
    else if (s.kind == chain::kWarp)  // whole frames only as well; never in place (chain::reads_elsewhere)
      e = l.nrows == frame_h && a != dst
              ? launch_warp(a, dst, w, frame_h, channels, s.warp.m, s.warp.mode, s.warp.interp, s.border, s.warp.value, stream)
              : hipErrorInvalidValue;
    else if (s.kind == chain::kResize)  // whole frames only; never in place; the launch carries both sizes
      e = l.a_w && a != dst ? launch_resize(a, dst, l.a_w, l.a_h, channels, s.resize.dw, s.resize.dh, s.resize.fx, s.resize.fy,
                                            s.resize.interp, stream)
                            : hipErrorInvalidValue;
    else
      e = hipErrorInvalidValue;  // no kernel for the kind: validate() lets none through
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace vf

namespace {

int chain_program(vf_ctx *ctx, const char *fn, const vf_step *steps, int nsteps, int channels, vf::chain::Program *out,
                  std::vector<uint64_t> *masks);  // below, with the chains

// The host path of every program, a vf_step list: its checks and the frames', the bands
// (vf_conv_bands.h) for the program's vertical reach, and per fill of the staging buffers upload,
// the band's launches, download, wait.
// One band: value v's row y sits at (its buffer) + (y - band.s0) * row, every buffer at the one row
// origin, so an in-place step is dst == operand exactly.  Buffer 0 is the band's upload, the others
// are the context's scratch (the pieces of one fill share it: they run in order on the one
// stream); the last step writes the band's output rows straight into dout.
int program_frames_host(vf_ctx *ctx, const char *fn, const uint8_t *const *srcs, uint8_t *const *dsts,
                        const int *widths, const int *heights, int n, int channels, const vf_step *steps, int nsteps) {
  vf::chain::Program prog;
  std::vector<uint64_t> masks;
  int rc = chain_program(ctx, fn, steps, nsteps, channels, &prog, &masks);
  if (rc != VF_OK) return rc;
  const int ry = vf::chain::reach(prog);
  const bool whole = vf::chain::whole_frame(prog);  // a level step: every frame is one band, or refused
  const bool sized = vf::chain::has_resize(prog);   // a resize step: a size per value, the result's is not the frame's
  std::vector<std::vector<vf::chain::Size>> sizes((size_t)(n > 0 ? n : 0));  // sized: of frame i's values
  if (n < 0) return set_err(ctx, VF_E_INVALID, 0, "%s: n < 0", fn);
  if (n > 0 && (!srcs || !dsts || !widths || !heights)) return set_err(ctx, VF_E_INVALID, 0, "%s: NULL array", fn);
  // one upload + launch + download per band (vf_conv_bands.h); most frames are one band
  struct Piece {
    int frame;
    vf::conv::Band b;
    const uint8_t *halo;  // in-place frames: the band's rows [s0, y0), saved before a download overwrote them
  };
  std::vector<Piece> pieces;
  std::vector<std::vector<uint8_t>> saved;
  const size_t cap = ctx->raw_cap;
  for (int i = 0; i < n; ++i) {
    if (widths[i] == 0 && heights[i] == 0) continue;  // the empty frame
    if ((rc = check_frame_shape(ctx, fn, widths[i], heights[i], channels)) != VF_OK) return rc;
    if (!srcs[i] || !dsts[i]) return set_err(ctx, VF_E_INVALID, 0, "%s: frame %d has a NULL buffer", fn, i);
    const size_t row = (size_t)widths[i] * (size_t)channels;
    std::vector<vf::conv::Band> bs;
    if (sized) {
      std::string why;
      if (!vf::chain::value_sizes(prog, widths[i], heights[i], &sizes[(size_t)i], &why))
        return set_err(ctx, VF_E_INVALID, 0, "%s: frame %d: %s", fn, i, why.c_str());
      const vf::chain::Size out = sizes[(size_t)i].back();
      const size_t in_bytes = row * (size_t)heights[i], out_bytes = (size_t)out.w * (size_t)out.h * (size_t)channels;
      if (out.w == widths[i] && out.h == heights[i]) {
        if (overlaps_partially(srcs[i], dsts[i], in_bytes))
          return set_err(ctx, VF_E_INVALID, 0, "%s: frame %d src/dst partially overlap", fn, i);
      } else if (srcs[i] < dsts[i] + out_bytes && dsts[i] < srcs[i] + in_bytes) {
        return set_err(ctx, VF_E_INVALID, 0, "%s: frame %d: src (%d x %d) and dst (%d x %d) overlap; frames of two sizes do not share memory",
                       fn, i, widths[i], heights[i], out.w, out.h);
      }
      for (size_t v = 0; v < sizes[(size_t)i].size(); ++v) {
        const vf::chain::Size z = sizes[(size_t)i][v];
        if ((size_t)z.w * (size_t)z.h * (size_t)channels > cap)
          return set_err(ctx, VF_E_INVALID, 0,
                         "%s: frame %d: value %zu of %d x %d (%zu bytes) does not fit the context's %zu-byte staging (a resize "
                         "step reads the whole frame: it is not cut into bands)",
                         fn, i, v, z.w, z.h, (size_t)z.w * (size_t)z.h * (size_t)channels, cap);
      }
    } else if (overlaps_partially(srcs[i], dsts[i], row * (size_t)heights[i])) {
      return set_err(ctx, VF_E_INVALID, 0, "%s: frame %d src/dst partially overlap", fn, i);
    }
    if (whole) {
      std::string why;
      for (const vf::chain::Step &s : prog.steps) {
        // the step's operand: the frame, or under a resize step the value's own size
        const uint64_t vw = (uint64_t)(sized ? sizes[(size_t)i][(size_t)s.a].w : widths[i]),
                       vh = (uint64_t)(sized ? sizes[(size_t)i][(size_t)s.a].h : heights[i]);
        if (s.kind == vf::chain::kLevel && !vf::level::pixels_ok(vw * vh, s.mask, s.link, channels, &why))
          return set_err(ctx, VF_E_INVALID, 0, "%s: frame %d: %s", fn, i, why.c_str());
      }
      for (const vf::chain::Step &s : prog.steps) {
        const uint64_t vw = (uint64_t)(sized ? sizes[(size_t)i][(size_t)s.a].w : widths[i]),
                       vh = (uint64_t)(sized ? sizes[(size_t)i][(size_t)s.a].h : heights[i]);
        if (s.kind == vf::chain::kClahe && !vf::clahe::frame_ok(vw, vh, s.tiles_x, s.tiles_y, &why))
          return set_err(ctx, VF_E_INVALID, 0, "%s: frame %d: %s", fn, i, why.c_str());
      }
      for (const vf::chain::Step &s : prog.steps) {
        const uint64_t vw = (uint64_t)(sized ? sizes[(size_t)i][(size_t)s.a].w : widths[i]),
                       vh = (uint64_t)(sized ? sizes[(size_t)i][(size_t)s.a].h : heights[i]);
        if (s.kind == vf::chain::kWarp && !vf::warp::frame_ok(vw, vh, s.warp.mode, s.warp.m, &why))
          return set_err(ctx, VF_E_INVALID, 0, "%s: frame %d: %s", fn, i, why.c_str());
      }
      if (!sized && row * (size_t)heights[i] > cap)  // sized: every value was checked above, the frame among them
        return set_err(ctx, VF_E_INVALID, 0,
                       "%s: frame %d: %d rows of %zu bytes do not fit the context's %zu-byte staging (a level step "
                       "reads the whole frame: it is not cut into bands)",
                       fn, i, heights[i], row, cap);
      bs.push_back(vf::conv::Band{0, heights[i], 0, heights[i]});
    } else if (!vf::conv::bands(widths[i], heights[i], channels, ry, cap, &bs))
      return set_err(ctx, VF_E_INVALID, 0, "%s: frame %d: %d rows of %zu bytes do not fit the context's %zu-byte staging",
                     fn, i, 2 * ry + 1, row, cap);
    for (const vf::conv::Band &b : bs) {
      const uint8_t *halo = nullptr;
      if (srcs[i] == dsts[i] && b.s0 < b.y0) {  // these rows are output rows of the band before
        saved.emplace_back(srcs[i] + (size_t)b.s0 * row, srcs[i] + (size_t)b.y0 * row);
        halo = saved.back().data();
      }
      pieces.push_back(Piece{i, b, halo});
    }
  }
  if (pieces.empty()) return VF_OK;
  std::lock_guard<std::mutex> lk(ctx->raw_mu);
  VF_HIP(ctx, hipSetDevice(ctx->device));
  const size_t alloc = ((cap + 15 + 15) & ~(size_t)15);
  if ((rc = raw_staging(ctx, fn, alloc)) != VF_OK) return rc;
  // Buffer 0 is a piece's upload slot in raw_din, as large as the frame and followed by the next piece's.  Under a
  // resize step a later value may be larger than the frame, so buffer 0 is kept for value 0 alone (keep_input):
  // every other value lives in a scratch buffer of `alloc` bytes, and every value was checked against cap above.
  const vf::chain::Buffers bufs = vf::chain::assign_buffers(prog, sized);
  while ((int)ctx->raw_scratch.size() < vf::chain::scratch_buffers(bufs, prog, true)) {
    void *p = nullptr;
    VF_HIP(ctx, hipMalloc(&p, alloc));
    ctx->raw_scratch.push_back(static_cast<uint8_t *>(p));
  }
  if (whole && ctx->level_hist_bytes < vf::chain::whole_frame_scratch_bytes(prog)) {
    // nothing is queued on raw_stream between calls (each ends with a wait), so the old words are idle
    if (ctx->level_hist) VF_HIP(ctx, hipFree(ctx->level_hist));
    ctx->level_hist = nullptr, ctx->level_hist_bytes = 0;
    void *p = nullptr;
    VF_HIP(ctx, hipMalloc(&p, vf::chain::whole_frame_scratch_bytes(prog)));
    ctx->level_hist = static_cast<uint32_t *>(p);
    ctx->level_hist_bytes = vf::chain::whole_frame_scratch_bytes(prog);
  }
  uint8_t *base[vf::chain::kMaxSteps + 1] = {};  // base[0]: each piece's upload; a value per step at the most
  std::copy(ctx->raw_scratch.begin(), ctx->raw_scratch.end(), base + 1);
  const int form = vf::conv_form_env();
  hipStream_t st = ctx->raw_stream;
  std::vector<size_t> at(pieces.size());
  for (size_t i = 0; i < pieces.size();) {
    // one fill of the buffers: upload and filter the bands that fit, download them, wait
    size_t cin = 0, cout = 0, j = i;
    for (; j < pieces.size(); ++j) {
      const Piece &p = pieces[j];
      const size_t row = (size_t)widths[p.frame] * (size_t)channels;
      const size_t in_bytes = (size_t)(p.b.s1 - p.b.s0) * row;
      const size_t out_bytes = sized ? (size_t)sizes[(size_t)p.frame].back().w * (size_t)sizes[(size_t)p.frame].back().h * (size_t)channels
                                     : (size_t)(p.b.y1 - p.b.y0) * row;
      if (cin + in_bytes > alloc || cout + out_bytes > alloc) break;
      uint8_t *din = ctx->raw_din + cin, *dout = ctx->raw_dout + cout;
      const uint8_t *src = srcs[p.frame];
      size_t head = 0;
      if (p.halo) {
        head = (size_t)(p.b.y0 - p.b.s0) * row;
        VF_HIP(ctx, hipMemcpyAsync(din, p.halo, head, hipMemcpyHostToDevice, st));
      }
      VF_HIP(ctx, hipMemcpyAsync(din + head, src + (size_t)p.b.s0 * row + head, in_bytes - head, hipMemcpyHostToDevice, st));
      base[0] = din;
      const int w = widths[p.frame], h = heights[p.frame];
      VF_HIP(ctx, vf::run_launches(prog, masks.data(),
                                   sized ? vf::chain::frame_launches(prog, bufs, sizes[(size_t)p.frame], true)
                                         : vf::chain::band_launches(prog, bufs, h, p.b.y0, p.b.y1, p.b.s0, true),
                                   base, dout, w, channels, h, form, whole ? ctx->level_hist : nullptr, ctx->cfg, st));
      at[j] = cout;
      cin += (in_bytes + 15) & ~(size_t)15;
      cout += (out_bytes + 15) & ~(size_t)15;
    }
    for (size_t k = i; k < j; ++k) {
      const Piece &p = pieces[k];
      const size_t row = (size_t)widths[p.frame] * (size_t)channels;
      if (sized) {  // one band, the result's size
        const vf::chain::Size out = sizes[(size_t)p.frame].back();
        VF_HIP(ctx, hipMemcpyAsync(dsts[p.frame], ctx->raw_dout + at[k], (size_t)out.w * (size_t)out.h * (size_t)channels,
                                   hipMemcpyDeviceToHost, st));
        continue;
      }
      VF_HIP(ctx, hipMemcpyAsync(dsts[p.frame] + (size_t)p.b.y0 * row, ctx->raw_dout + at[k],
                                 (size_t)(p.b.y1 - p.b.y0) * row, hipMemcpyDeviceToHost, st));
    }
    VF_HIP(ctx, hipStreamSynchronize(st));
    i = j;
  }
  return VF_OK;
}

}  // namespace

VF_EXPORT int vf_conv_frames_host(vf_ctx *ctx, const uint8_t *const *srcs, uint8_t *const *dsts, const int *widths,
                                  const int *heights, int n, int channels, const int16_t *weights, int kw, int kh,
                                  int shift, int border) {
  VF_CHECK_CTX(ctx);
  const char *fn = "vf_conv_frames_host";
  const int rc = check_kernel(ctx, fn, weights, kw, kh, shift, border);
  if (rc != VF_OK) return rc;
  const vf_step step{VF_STEP_CONV, 0, 0, 0, weights, kw, kh, shift, border, 0};  // a program of one step
  return program_frames_host(ctx, fn, srcs, dsts, widths, heights, n, channels, &step, 1);
}

// ---- rank filters (cv2.erode, cv2.dilate, cv2.medianBlur) on raw frames ---------------------------

namespace {

// The filter arguments every vf_rank_* / vf_jpeg_rank* entry point shares; *mask: the element's
// members, bit j * kw + i.
int check_rank(vf_ctx *ctx, const char *fn, int op, const uint8_t *element, int kw, int kh, int border, uint64_t *mask) {
  if (op != VF_RANK_ERODE && op != VF_RANK_DILATE && op != VF_RANK_MEDIAN)
    return set_err(ctx, VF_E_INVALID, 0, "%s: unknown op %d", fn, op);
  if (!element) return set_err(ctx, VF_E_INVALID, 0, "%s: element is NULL", fn);
  if (!vf::tile::sides_ok(kw, kh))
    return set_err(ctx, VF_E_INVALID, 0, "%s: a %d x %d element; sides are odd and at most %d", fn, kw, kh,
                   vf::conv::kMaxK);
  if (!vf::tile::border_ok(border)) return set_err(ctx, VF_E_INVALID, 0, "%s: unknown border %d", fn, border);
  *mask = vf::rank_mask(element, kw, kh);
  if (*mask == 0) return set_err(ctx, VF_E_INVALID, 0, "%s: an empty element (no member)", fn);
  if (op == VF_RANK_MEDIAN) {
    if (kw != kh || (kw != 3 && kw != 5))
      return set_err(ctx, VF_E_INVALID, 0, "%s: median over a %d x %d element; the square has side 3 or 5", fn, kw, kh);
    if (*mask != ((uint64_t)1 << (kw * kh)) - 1)
      return set_err(ctx, VF_E_INVALID, 0, "%s: median takes the full square, every entry a member", fn);
    if (border != VF_BORDER_REPLICATE)
      return set_err(ctx, VF_E_INVALID, 0, "%s: median with border %d; cv2.medianBlur replicates (border %d)", fn, border,
                     VF_BORDER_REPLICATE);
  }
  return VF_OK;
}

}  // namespace

VF_EXPORT int vf_rank_device(vf_ctx *ctx, const void *dsrc, void *ddst, int width, int height, int channels, int op,
                             const uint8_t *element, int kw, int kh, int border, void *stream) {
  VF_CHECK_CTX(ctx);
  uint64_t mask = 0;
  int rc = check_rank(ctx, "vf_rank_device", op, element, kw, kh, border, &mask);
  if (rc != VF_OK) return rc;
  if ((rc = check_device_frame(ctx, "vf_rank_device", dsrc, ddst, width, height, channels)) != VF_OK)
    return rc < 0 ? rc : VF_OK;
  VF_HIP(ctx, hipSetDevice(ctx->device));
  VF_HIP(ctx, vf::launch_rank(dsrc, ddst, width, channels, height, 0, height, 0, height, op, mask, kw, kh, border,
                              (hipStream_t)stream));
  return VF_OK;
}

VF_EXPORT int vf_rank_frames_host(vf_ctx *ctx, const uint8_t *const *srcs, uint8_t *const *dsts, const int *widths,
                                  const int *heights, int n, int channels, int op, const uint8_t *element, int kw, int kh,
                                  int border) {
  VF_CHECK_CTX(ctx);
  const char *fn = "vf_rank_frames_host";
  uint64_t mask = 0;
  const int rc = check_rank(ctx, fn, op, element, kw, kh, border, &mask);
  if (rc != VF_OK) return rc;
  const vf_step step{VF_STEP_RANK, 0, 0, op, element, kw, kh, 0, border, 0};  // a program of one step
  return program_frames_host(ctx, fn, srcs, dsts, widths, heights, n, channels, &step, 1);
}

// ---- colour matrix (cv2.transform) on raw 3-channel frames -----------------------------------------

namespace {

// The filter arguments every vf_mix_* / vf_jpeg_mix* entry point and a VF_STEP_MIX step share.
int check_mix(vf_ctx *ctx, const char *fn, const int32_t *m, int shift, int rounding) {
  if (!m) return set_err(ctx, VF_E_INVALID, 0, "%s: matrix is NULL", fn);
  if (shift < 0 || shift > 16) return set_err(ctx, VF_E_INVALID, 0, "%s: shift=%d outside 0..16", fn, shift);
  if (rounding != VF_ROUND_HALF_EVEN && rounding != VF_ROUND_HALF_UP)
    return set_err(ctx, VF_E_INVALID, 0, "%s: unknown rounding %d", fn, rounding);
  for (int c = 0; c < 3; ++c) {
    long sum = 0;
    for (int k = 0; k < 3; ++k) {
      const long v = m[4 * c + k];
      if (v < -32768 || v > 32767)
        return set_err(ctx, VF_E_INVALID, 0, "%s: weight M[%d][%d] = %ld does not fit int16", fn, c, k, v);
      sum += std::labs(v);
    }
    if (sum > 65536) return set_err(ctx, VF_E_INVALID, 0, "%s: row %d: sum|M| = %ld exceeds 65536", fn, c, sum);
    const long t = m[4 * c + 3], most = 255L << shift;
    if (t < -most || t > most)
      return set_err(ctx, VF_E_INVALID, 0, "%s: offset t[%d] = %ld; |t| is at most 255 * 2^shift = %ld", fn, c, t, most);
  }
  return VF_OK;
}

int check_mix_channels(vf_ctx *ctx, const char *fn, int channels) {
  if (channels == 1) return set_err(ctx, VF_E_INVALID, 0, "%s: a colour matrix on 1-channel frames", fn);
  if (channels != 3) return set_err(ctx, VF_E_INVALID, 0, "%s: channels=%d, a colour matrix takes 3", fn, channels);
  return VF_OK;
}

}  // namespace

VF_EXPORT size_t vf_mix_tile_bytes(void) { return vf::mix_tile_bytes(); }

VF_EXPORT int vf_mix_device(vf_ctx *ctx, const void *dsrc, void *ddst, size_t nbytes, const int32_t *matrix, int shift,
                            int rounding, void *stream) {
  VF_CHECK_CTX(ctx);
  const int rc = check_mix(ctx, "vf_mix_device", matrix, shift, rounding);
  if (rc != VF_OK) return rc;
  if (nbytes % 3 != 0)
    return set_err(ctx, VF_E_INVALID, 0, "vf_mix_device: %zu bytes are not whole 3-channel pixels", nbytes);
  if (nbytes == 0) return VF_OK;
  if (!dsrc || !ddst) return set_err(ctx, VF_E_INVALID, 0, "vf_mix_device: NULL buffer");
  if (overlaps_partially((const uint8_t *)dsrc, (const uint8_t *)ddst, nbytes))
    return set_err(ctx, VF_E_INVALID, 0, "vf_mix_device: src and dst partially overlap");
  VF_HIP(ctx, hipSetDevice(ctx->device));
  VF_HIP(ctx, vf::launch_mix(dsrc, ddst, nbytes, matrix, shift, rounding, ctx->cfg, (hipStream_t)stream));
  return VF_OK;
}

VF_EXPORT int vf_mix_frames_host(vf_ctx *ctx, const uint8_t *const *srcs, uint8_t *const *dsts, const int *widths,
                                 const int *heights, int n, int channels, const int32_t *matrix, int shift,
                                 int rounding) {
  VF_CHECK_CTX(ctx);
  const char *fn = "vf_mix_frames_host";
  int rc = check_mix(ctx, fn, matrix, shift, rounding);
  if (rc != VF_OK) return rc;
  if ((rc = check_mix_channels(ctx, fn, channels)) != VF_OK) return rc;
  const vf_step step{VF_STEP_MIX, 0, 0, rounding, matrix, 0, 0, shift, 0, 0};  // a program of one step
  return program_frames_host(ctx, fn, srcs, dsts, widths, heights, n, channels, &step, 1);
}

// ---- separable filter (cv2.sepFilter2D, cv2.blur, cv2.boxFilter) on raw frames ---------------------

namespace {

// The filter arguments every vf_sep_* / vf_jpeg_sep* entry point and a VF_STEP_SEP step share
// (vf_sep_plan.h has the limits).
int check_sep(vf_ctx *ctx, const char *fn, const int16_t *kx, int kw, const int16_t *ky, int kh, int shift, int divisor,
              int rounding, int border) {
  std::string why;
  if (!vf::sep::limits_ok(kx, kw, ky, kh, shift, divisor, rounding, border, &why))
    return set_err(ctx, VF_E_INVALID, 0, "%s: %s", fn, why.c_str());
  return VF_OK;
}

// A VF_STEP_SEP step's data for the taps of an entry point: the divisor, kx, ky as int32.
std::vector<int32_t> sep_step_data(const int16_t *kx, int kw, const int16_t *ky, int kh, int divisor) {
  std::vector<int32_t> d{divisor};
  d.insert(d.end(), kx, kx + kw);
  d.insert(d.end(), ky, ky + kh);
  return d;
}

}  // namespace

VF_EXPORT int vf_sep_tile(int kw, int kh, int *row_bytes, int *rows) {
  if (!vf::sep::side_ok(kw) || !vf::sep::side_ok(kh) || !row_bytes || !rows) return VF_E_INVALID;
  *row_bytes = vf::sep::kTileBytes;
  *rows = vf::sep_tile_rows(kh);
  return VF_OK;
}

VF_EXPORT int vf_sep_device(vf_ctx *ctx, const void *dsrc, void *ddst, int width, int height, int channels,
                            const int16_t *kx, int kw, const int16_t *ky, int kh, int shift, int divisor, int rounding,
                            int border, void *stream) {
  VF_CHECK_CTX(ctx);
  int rc = check_sep(ctx, "vf_sep_device", kx, kw, ky, kh, shift, divisor, rounding, border);
  if (rc != VF_OK) return rc;
  if ((rc = check_device_frame(ctx, "vf_sep_device", dsrc, ddst, width, height, channels)) != VF_OK)
    return rc < 0 ? rc : VF_OK;
  VF_HIP(ctx, hipSetDevice(ctx->device));
  VF_HIP(ctx, vf::launch_sep(dsrc, ddst, width, channels, height, 0, height, 0, height, kx, kw, ky, kh, shift, divisor,
                             rounding, border, vf::sep_form_env(), (hipStream_t)stream));
  return VF_OK;
}

VF_EXPORT int vf_sep_frames_host(vf_ctx *ctx, const uint8_t *const *srcs, uint8_t *const *dsts, const int *widths,
                                 const int *heights, int n, int channels, const int16_t *kx, int kw, const int16_t *ky,
                                 int kh, int shift, int divisor, int rounding, int border) {
  VF_CHECK_CTX(ctx);
  const char *fn = "vf_sep_frames_host";
  const int rc = check_sep(ctx, fn, kx, kw, ky, kh, shift, divisor, rounding, border);
  if (rc != VF_OK) return rc;
  const std::vector<int32_t> data = sep_step_data(kx, kw, ky, kh, divisor);
  const vf_step step{VF_STEP_SEP, 0, 0, rounding, data.data(), kw, kh, shift, border, 0};  // a program of one step
  return program_frames_host(ctx, fn, srcs, dsts, widths, heights, n, channels, &step, 1);
}

// ---- level filter (cv2.equalizeHist, auto-levels) and the histogram on raw frames ---------------------

namespace {

// The filter arguments every vf_level_* / vf_jpeg_level* entry point and a VF_STEP_LEVEL step share
// (vf_level_plan.h has the limits).
int check_level(vf_ctx *ctx, const char *fn, int rule, int mask, int link, int clip_lo, int clip_hi, int channels) {
  std::string why;
  if (!vf::level::limits_ok(rule, mask, link, clip_lo, clip_hi, channels, &why))
    return set_err(ctx, VF_E_INVALID, 0, "%s: %s", fn, why.c_str());
  return VF_OK;
}

}  // namespace

VF_EXPORT int vf_hist_device(vf_ctx *ctx, const void *dsrc, size_t nbytes, int channels, uint32_t *dhist, void *stream) {
  VF_CHECK_CTX(ctx);
  const char *fn = "vf_hist_device";
  const int rc = check_channels(ctx, fn, channels);
  if (rc != VF_OK) return rc;
  if (nbytes % (size_t)channels != 0)
    return set_err(ctx, VF_E_INVALID, 0, "%s: %zu bytes are not whole %d-channel pixels", fn, nbytes, channels);
  std::string why;
  if (!vf::level::pixels_ok(nbytes / (size_t)channels, 0, 0, channels, &why))
    return set_err(ctx, VF_E_INVALID, 0, "%s: %s", fn, why.c_str());
  if (!dhist) return set_err(ctx, VF_E_INVALID, 0, "%s: hist is NULL", fn);
  if ((uintptr_t)dhist & 3) return set_err(ctx, VF_E_INVALID, 0, "%s: hist is not 4-byte aligned", fn);
  if (nbytes != 0 && !dsrc) return set_err(ctx, VF_E_INVALID, 0, "%s: NULL buffer", fn);
  VF_HIP(ctx, hipSetDevice(ctx->device));
  VF_HIP(ctx, hipMemsetAsync(dhist, 0, (size_t)channels * 256 * sizeof(uint32_t), (hipStream_t)stream));
  VF_HIP(ctx, vf::launch_hist(dsrc, nbytes, channels, dhist, ctx->cfg, (hipStream_t)stream));
  return VF_OK;
}

VF_EXPORT int vf_hist_frames_host(vf_ctx *ctx, const uint8_t *const *srcs, const size_t *nbytes, int n, int channels,
                                  uint32_t *hists) {
  VF_CHECK_CTX(ctx);
  const char *fn = "vf_hist_frames_host";
  int rc = check_channels(ctx, fn, channels);
  if (rc != VF_OK) return rc;
  if (n < 0) return set_err(ctx, VF_E_INVALID, 0, "%s: n < 0", fn);
  if (n > 0 && (!srcs || !nbytes || !hists)) return set_err(ctx, VF_E_INVALID, 0, "%s: NULL array", fn);
  for (int i = 0; i < n; ++i) {
    if (nbytes[i] % (size_t)channels != 0)
      return set_err(ctx, VF_E_INVALID, 0, "%s: frame %d: %zu bytes are not whole %d-channel pixels", fn, i, nbytes[i],
                     channels);
    std::string why;
    if (!vf::level::pixels_ok(nbytes[i] / (size_t)channels, 0, 0, channels, &why))
      return set_err(ctx, VF_E_INVALID, 0, "%s: frame %d: %s", fn, i, why.c_str());
    if (nbytes[i] != 0 && !srcs[i]) return set_err(ctx, VF_E_INVALID, 0, "%s: frame %d has a NULL buffer", fn, i);
  }
  if (n == 0) return VF_OK;
  const size_t words = (size_t)channels * 256;
  std::lock_guard<std::mutex> lk(ctx->raw_mu);
  VF_HIP(ctx, hipSetDevice(ctx->device));
  const size_t cap = ctx->raw_cap, alloc = ((cap + 15 + 15) & ~(size_t)15);
  if ((rc = raw_staging(ctx, fn, alloc)) != VF_OK) return rc;
  // the frames' words sit in raw_dout, a group of as many frames as it holds at a time; a frame's
  // bytes go through raw_din in pieces of whole pixels that keep the caller's offset mod 16, one
  // fill of raw_din after the other, every piece added to the frame's words
  const size_t group = alloc / (words * sizeof(uint32_t));
  if (group == 0) return set_err(ctx, VF_E_INVALID, 0, "%s: the context's %zu-byte staging holds no histogram", fn, cap);
  const size_t piece_max = cap / 48 * 48;  // whole pixels and whole 16-B vectors
  if (piece_max == 0) return set_err(ctx, VF_E_INVALID, 0, "%s: the context's %zu-byte staging holds no pixel", fn, cap);
  hipStream_t st = ctx->raw_stream;
  uint32_t *dh = reinterpret_cast<uint32_t *>(ctx->raw_dout);
  for (size_t g0 = 0; g0 < (size_t)n; g0 += group) {
    const size_t g1 = std::min((size_t)n, g0 + group);
    VF_HIP(ctx, hipMemsetAsync(dh, 0, (g1 - g0) * words * sizeof(uint32_t), st));
    size_t cur = 0;
    for (size_t i = g0; i < g1; ++i) {
      for (size_t off = 0; off < nbytes[i];) {
        const size_t len = std::min(piece_max, nbytes[i] - off);
        const size_t room = (len + 15 + 15) & ~(size_t)15;
        if (cur + room > alloc) {  // raw_din is full: let its pieces be counted before they are overwritten
          VF_HIP(ctx, hipStreamSynchronize(st));
          cur = 0;
        }
        uint8_t *din = ctx->raw_din + cur + ((uintptr_t)(srcs[i] + off) & 15);
        VF_HIP(ctx, hipMemcpyAsync(din, srcs[i] + off, len, hipMemcpyHostToDevice, st));
        VF_HIP(ctx, vf::launch_hist(din, len, channels, dh + (i - g0) * words, ctx->cfg, st));
        cur += room;
        off += len;
      }
    }
    VF_HIP(ctx, hipMemcpyAsync(hists + g0 * words, dh, (g1 - g0) * words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    VF_HIP(ctx, hipStreamSynchronize(st));
  }
  return VF_OK;
}

VF_EXPORT int vf_level_device(vf_ctx *ctx, const void *dsrc, void *ddst, int width, int height, int channels, int rule,
                              int mask, int link, int clip_lo, int clip_hi, void *stream) {
  VF_CHECK_CTX(ctx);
  const char *fn = "vf_level_device";
  int rc = check_channels(ctx, fn, channels);
  if (rc != VF_OK) return rc;
  if ((rc = check_level(ctx, fn, rule, mask, link, clip_lo, clip_hi, channels)) != VF_OK) return rc;
  if (width == 0 && height == 0) return VF_OK;  // the empty frame
  if ((rc = check_frame_shape(ctx, fn, width, height, channels)) != VF_OK) return rc;
  std::string why;
  if (!vf::level::pixels_ok((uint64_t)width * (uint64_t)height, mask, link, channels, &why))
    return set_err(ctx, VF_E_INVALID, 0, "%s: %s", fn, why.c_str());
  if (!dsrc || !ddst) return set_err(ctx, VF_E_INVALID, 0, "%s: NULL buffer", fn);
  const size_t nbytes = (size_t)width * (size_t)channels * (size_t)height;
  if (overlaps_partially((const uint8_t *)dsrc, (const uint8_t *)ddst, nbytes))
    return set_err(ctx, VF_E_INVALID, 0, "%s: src and dst partially overlap", fn);
  VF_HIP(ctx, hipSetDevice(ctx->device));
  {
    std::lock_guard<std::mutex> lk(ctx->level_mu);
    if (!ctx->level_dev_hist) {
      void *p = nullptr;
      VF_HIP(ctx, hipMalloc(&p, vf::level::kHistWords * sizeof(uint32_t)));
      ctx->level_dev_hist = static_cast<uint32_t *>(p);
    }
  }
  VF_HIP(ctx, vf::launch_level(dsrc, ddst, nbytes, channels, rule, mask, link, clip_lo, clip_hi, ctx->level_dev_hist,
                               ctx->cfg, (hipStream_t)stream));
  return VF_OK;
}

VF_EXPORT int vf_level_frames_host(vf_ctx *ctx, const uint8_t *const *srcs, uint8_t *const *dsts, const int *widths,
                                   const int *heights, int n, int channels, int rule, int mask, int link, int clip_lo,
                                   int clip_hi) {
  VF_CHECK_CTX(ctx);
  const char *fn = "vf_level_frames_host";
  int rc = check_channels(ctx, fn, channels);
  if (rc != VF_OK) return rc;
  if ((rc = check_level(ctx, fn, rule, mask, link, clip_lo, clip_hi, channels)) != VF_OK) return rc;
  const int32_t data[4] = {mask, link, clip_lo, clip_hi};
  const vf_step step{VF_STEP_LEVEL, 0, 0, rule, data, 0, 0, 0, 0, 0};  // a program of one step
  return program_frames_host(ctx, fn, srcs, dsts, widths, heights, n, channels, &step, 1);
}

// ---- CLAHE (cv2.createCLAHE(...).apply) on raw frames ---------------------------------------------------

namespace {

// The filter arguments every vf_clahe_* / vf_jpeg_clahe* entry point and a VF_STEP_CLAHE step share
// (vf_clahe_plan.h has the limits).
int check_clahe(vf_ctx *ctx, const char *fn, int clip_q8, int tiles_x, int tiles_y, int mask, int channels) {
  std::string why;
  if (!vf::clahe::limits_ok(clip_q8, tiles_x, tiles_y, mask, channels, &why))
    return set_err(ctx, VF_E_INVALID, 0, "%s: %s", fn, why.c_str());
  return VF_OK;
}

}  // namespace

VF_EXPORT int vf_clahe_device(vf_ctx *ctx, const void *dsrc, void *ddst, int width, int height, int channels, int clip_q8,
                              int tiles_x, int tiles_y, int mask, void *stream) {
  VF_CHECK_CTX(ctx);
  const char *fn = "vf_clahe_device";
  int rc = check_channels(ctx, fn, channels);
  if (rc != VF_OK) return rc;
  if ((rc = check_clahe(ctx, fn, clip_q8, tiles_x, tiles_y, mask, channels)) != VF_OK) return rc;
  if (width == 0 && height == 0) return VF_OK;  // the empty frame
  if ((rc = check_frame_shape(ctx, fn, width, height, channels)) != VF_OK) return rc;
  std::string why;
  if (!vf::clahe::frame_ok((uint64_t)width, (uint64_t)height, tiles_x, tiles_y, &why))
    return set_err(ctx, VF_E_INVALID, 0, "%s: %s", fn, why.c_str());
  if (!dsrc || !ddst) return set_err(ctx, VF_E_INVALID, 0, "%s: NULL buffer", fn);
  const size_t nbytes = (size_t)width * (size_t)channels * (size_t)height;
  if (overlaps_partially((const uint8_t *)dsrc, (const uint8_t *)ddst, nbytes))
    return set_err(ctx, VF_E_INVALID, 0, "%s: src and dst partially overlap", fn);
  VF_HIP(ctx, hipSetDevice(ctx->device));
  {
    std::lock_guard<std::mutex> lk(ctx->level_mu);
    if (!ctx->clahe_dev) VF_HIP(ctx, hipMalloc(&ctx->clahe_dev, vf::clahe::kScratchBytes));
  }
  VF_HIP(ctx, vf::launch_clahe(dsrc, ddst, width, height, channels, clip_q8, tiles_x, tiles_y, mask, ctx->clahe_dev,
                               (hipStream_t)stream));
  return VF_OK;
}

VF_EXPORT int vf_clahe_frames_host(vf_ctx *ctx, const uint8_t *const *srcs, uint8_t *const *dsts, const int *widths,
                                   const int *heights, int n, int channels, int clip_q8, int tiles_x, int tiles_y,
                                   int mask) {
  VF_CHECK_CTX(ctx);
  const char *fn = "vf_clahe_frames_host";
  int rc = check_channels(ctx, fn, channels);
  if (rc != VF_OK) return rc;
  if ((rc = check_clahe(ctx, fn, clip_q8, tiles_x, tiles_y, mask, channels)) != VF_OK) return rc;
  const int32_t data[4] = {mask, clip_q8, tiles_x, tiles_y};
  const vf_step step{VF_STEP_CLAHE, 0, 0, 0, data, 0, 0, 0, 0, 0};  // a program of one step
  return program_frames_host(ctx, fn, srcs, dsts, widths, heights, n, channels, &step, 1);
}

// ---- the affine warp (cv2.warpAffine, cv2.flip) on raw frames ------------------------------------------

namespace {

// The filter arguments every vf_warp_* / vf_jpeg_warp* entry point and a VF_STEP_WARP step share
// (vf_warp_plan.h has the limits).
int check_warp(vf_ctx *ctx, const char *fn, const double *m, int mode, int interp, int border, const int *value,
               int channels) {
  std::string why;
  if (!vf::warp::limits_ok(m, mode, interp, border, value, channels, &why))
    return set_err(ctx, VF_E_INVALID, 0, "%s: %s", fn, why.c_str());
  return VF_OK;
}

// A VF_STEP_WARP step's data (include/vfilter.h): six float64, then {mode, interp, value B, G, R, 0}.
struct WarpStepData {
  double m[6];
  int32_t i[6];
};
static_assert(sizeof(WarpStepData) == vf::warp::kStepBytes, "the step's data is packed");

WarpStepData warp_step_data(const double *m, int mode, int interp, const int *value) {
  WarpStepData d = {};
  if (m && mode == vf::warp::kAffine) std::memcpy(d.m, m, sizeof d.m);
  d.i[0] = mode, d.i[1] = interp, d.i[2] = value[0], d.i[3] = value[1], d.i[4] = value[2];
  return d;
}

}  // namespace

VF_EXPORT int vf_warp_device(vf_ctx *ctx, const void *dsrc, void *ddst, int width, int height, int channels, const double *m,
                             int mode, int interp, int border, const int *value, void *stream) {
  VF_CHECK_CTX(ctx);
  const char *fn = "vf_warp_device";
  int rc = check_channels(ctx, fn, channels);
  if (rc != VF_OK) return rc;
  if ((rc = check_warp(ctx, fn, m, mode, interp, border, value, channels)) != VF_OK) return rc;
  if ((rc = check_device_frame(ctx, fn, dsrc, ddst, width, height, channels)) != VF_OK) return rc < 0 ? rc : VF_OK;
  std::string why;
  if (!vf::warp::frame_ok((uint64_t)width, (uint64_t)height, mode, m, &why))
    return set_err(ctx, VF_E_INVALID, 0, "%s: %s", fn, why.c_str());
  const uint8_t v[3] = {(uint8_t)value[0], (uint8_t)value[1], (uint8_t)value[2]};
  VF_HIP(ctx, hipSetDevice(ctx->device));
  VF_HIP(ctx, vf::launch_warp(dsrc, ddst, width, height, channels, m, mode, interp, border, v, (hipStream_t)stream));
  return VF_OK;
}

VF_EXPORT int vf_warp_frames_host(vf_ctx *ctx, const uint8_t *const *srcs, uint8_t *const *dsts, const int *widths,
                                  const int *heights, int n, int channels, const double *m, int mode, int interp,
                                  int border, const int *value) {
  VF_CHECK_CTX(ctx);
  const char *fn = "vf_warp_frames_host";
  int rc = check_channels(ctx, fn, channels);
  if (rc != VF_OK) return rc;
  if ((rc = check_warp(ctx, fn, m, mode, interp, border, value, channels)) != VF_OK) return rc;
  const WarpStepData data = warp_step_data(m, mode, interp, value);
  const vf_step step{VF_STEP_WARP, 0, 0, 0, &data, 0, 0, 0, border, 0};  // a program of one step
  return program_frames_host(ctx, fn, srcs, dsts, widths, heights, n, channels, &step, 1);
}

// ---- the resize (cv2.resize) on raw frames -------------------------------------------------------------

namespace {

// The filter arguments every vf_resize_* / vf_jpeg_resize* entry point and a VF_STEP_RESIZE step share
// (vf_resize_plan.h has the limits).
int check_resize(vf_ctx *ctx, const char *fn, int dw, int dh, double fx, double fy, int interp, int channels) {
  std::string why;
  if (!vf::resize::limits_ok(dw, dh, fx, fy, interp, channels, &why))
    return set_err(ctx, VF_E_INVALID, 0, "%s: %s", fn, why.c_str());
  return VF_OK;
}

// A VF_STEP_RESIZE step's data (include/vfilter.h): two float64, then {dw, dh, interp, 0}.
struct ResizeStepData {
  double f[2];
  int32_t i[4];
};
static_assert(sizeof(ResizeStepData) == vf::resize::kStepBytes, "the step's data is packed");

ResizeStepData resize_step_data(int dw, int dh, double fx, double fy, int interp) {
  ResizeStepData d = {};
  d.f[0] = fx, d.f[1] = fy, d.i[0] = dw, d.i[1] = dh, d.i[2] = interp;
  return d;
}

}  // namespace

VF_EXPORT int vf_resize_out_size(vf_ctx *ctx, int width, int height, int dw, int dh, double fx, double fy, int interp,
                                 int *out_w, int *out_h) {
  VF_CHECK_CTX(ctx);
  const char *fn = "vf_resize_out_size";
  if (!out_w || !out_h) return set_err(ctx, VF_E_INVALID, 0, "%s: NULL result", fn);
  int rc = check_resize(ctx, fn, dw, dh, fx, fy, interp, 1);
  if (rc != VF_OK) return rc;
  if (width == 0 && height == 0) {  // the empty frame stays empty
    *out_w = *out_h = 0;
    return VF_OK;
  }
  if ((rc = check_frame_shape(ctx, fn, width, height, 1)) != VF_OK) return rc;
  vf::resize::Plan p;
  std::string why;
  if (!vf::resize::frame_ok((uint64_t)width, (uint64_t)height, dw, dh, fx, fy, interp, &p, &why))
    return set_err(ctx, VF_E_INVALID, 0, "%s: %s", fn, why.c_str());
  *out_w = p.dw, *out_h = p.dh;
  return VF_OK;
}

VF_EXPORT int vf_resize_device(vf_ctx *ctx, const void *dsrc, void *ddst, int width, int height, int channels, int dw, int dh,
                               double fx, double fy, int interp, void *stream) {
  VF_CHECK_CTX(ctx);
  const char *fn = "vf_resize_device";
  int rc = check_channels(ctx, fn, channels);
  if (rc != VF_OK) return rc;
  if ((rc = check_resize(ctx, fn, dw, dh, fx, fy, interp, channels)) != VF_OK) return rc;
  if (width == 0 && height == 0) return VF_OK;
  if ((rc = check_frame_shape(ctx, fn, width, height, channels)) != VF_OK) return rc;
  vf::resize::Plan p;
  std::string why;
  if (!vf::resize::frame_ok((uint64_t)width, (uint64_t)height, dw, dh, fx, fy, interp, &p, &why))
    return set_err(ctx, VF_E_INVALID, 0, "%s: %s", fn, why.c_str());
  if (!dsrc || !ddst) return set_err(ctx, VF_E_INVALID, 0, "%s: NULL buffer", fn);
  const size_t in_bytes = (size_t)width * (size_t)channels * (size_t)height, out_bytes = (size_t)p.dw * (size_t)channels * (size_t)p.dh;
  const uint8_t *s = (const uint8_t *)dsrc, *d = (const uint8_t *)ddst;
  if (s < d + out_bytes && d < s + in_bytes)  // out of place only: the two frames are not of one size
    return set_err(ctx, VF_E_INVALID, 0, "%s: src and dst overlap", fn);
  VF_HIP(ctx, hipSetDevice(ctx->device));
  VF_HIP(ctx, vf::launch_resize(dsrc, ddst, width, height, channels, dw, dh, fx, fy, interp, (hipStream_t)stream));
  return VF_OK;
}

VF_EXPORT int vf_resize_frames_host(vf_ctx *ctx, const uint8_t *const *srcs, uint8_t *const *dsts, const int *widths,
                                    const int *heights, int n, int channels, int dw, int dh, double fx, double fy,
                                    int interp) {
  VF_CHECK_CTX(ctx);
  const char *fn = "vf_resize_frames_host";
  int rc = check_channels(ctx, fn, channels);
  if (rc != VF_OK) return rc;
  if ((rc = check_resize(ctx, fn, dw, dh, fx, fy, interp, channels)) != VF_OK) return rc;
  const ResizeStepData data = resize_step_data(dw, dh, fx, fy, interp);
  const vf_step step{VF_STEP_RESIZE, 0, 0, 0, &data, 0, 0, 0, 0, 0};  // a program of one step
  return program_frames_host(ctx, fn, srcs, dsts, widths, heights, n, channels, &step, 1);
}

// ---- filter chains: a program of table / conv / rank / binary / mix / sep / level / clahe / warp / resize steps on raw frames

namespace {

// A vf_step list as a validated, folded program: every step through its single-filter check, then
// the structure (vf_chain_plan.h).  masks[i]: the element of step i + 1 of the FOLDED program.
int chain_program(vf_ctx *ctx, const char *fn, const vf_step *steps, int nsteps, int channels, vf::chain::Program *out,
                  std::vector<uint64_t> *masks) {
  int rc = check_channels(ctx, fn, channels);
  if (rc != VF_OK) return rc;
  if (nsteps < 1 || nsteps > VF_CHAIN_MAX_STEPS)
    return set_err(ctx, VF_E_INVALID, 0, "%s: a program of %d steps; it has 1 to %d", fn, nsteps, VF_CHAIN_MAX_STEPS);
  if (!steps) return set_err(ctx, VF_E_INVALID, 0, "%s: steps is NULL", fn);
  vf::chain::Program p;
  for (int i = 0; i < nsteps; ++i) {
    const vf_step &in = steps[i];
    vf::chain::Step s;
    s.kind = in.kind;
    s.a = in.a;
    s.b = in.b;
    s.op = in.op;
    char at[96];
    std::snprintf(at, sizeof at, "%s: step %d", fn, i + 1);
    if (in.kind == VF_STEP_TABLE) {
      if ((rc = check_table(ctx, at, static_cast<const uint8_t *>(in.data), in.channels)) != VF_OK) return rc;
      s.channels = in.channels;
      const uint8_t *t = static_cast<const uint8_t *>(in.data);
      s.table.assign(t, t + 256 * (size_t)in.channels);
    } else if (in.kind == VF_STEP_CONV) {
      const int16_t *w = static_cast<const int16_t *>(in.data);
      if ((rc = check_kernel(ctx, at, w, in.kw, in.kh, in.shift, in.border)) != VF_OK) return rc;
      s.kw = in.kw, s.kh = in.kh, s.shift = in.shift, s.border = in.border;
      s.weights.assign(w, w + (size_t)in.kw * in.kh);
    } else if (in.kind == VF_STEP_RANK) {
      const uint8_t *e = static_cast<const uint8_t *>(in.data);
      uint64_t mask = 0;
      if ((rc = check_rank(ctx, at, in.op, e, in.kw, in.kh, in.border, &mask)) != VF_OK) return rc;
      s.kw = in.kw, s.kh = in.kh, s.border = in.border;
      s.element.assign(e, e + (size_t)in.kw * in.kh);
    } else if (in.kind == VF_STEP_MIX) {
      const int32_t *m = static_cast<const int32_t *>(in.data);
      if ((rc = check_mix(ctx, at, m, in.shift, in.op)) != VF_OK) return rc;
      s.shift = in.shift;
      s.matrix.assign(m, m + 12);
    } else if (in.kind == VF_STEP_SEP) {
      // data: the divisor (0 or 1: none), kw horizontal taps, kh vertical taps, int32 each
      const int32_t *d = static_cast<const int32_t *>(in.data);
      if (!d) return set_err(ctx, VF_E_INVALID, 0, "%s: taps are NULL", at);
      if (!vf::sep::side_ok(in.kw) || !vf::sep::side_ok(in.kh))
        return set_err(ctx, VF_E_INVALID, 0, "%s: a %d x %d separable kernel; tap counts are odd and at most %d", at, in.kw,
                       in.kh, vf::sep::kMaxSide);
      for (int k = 1; k <= in.kw + in.kh; ++k)
        if (d[k] < -32768 || d[k] > 32767)
          return set_err(ctx, VF_E_INVALID, 0, "%s: tap %d = %d does not fit int16", at, k - 1, d[k]);
      s.taps_x.assign(d + 1, d + 1 + in.kw);
      s.taps_y.assign(d + 1 + in.kw, d + 1 + in.kw + in.kh);
      s.divisor = d[0] == 0 ? 1 : d[0];
      if ((rc = check_sep(ctx, at, s.taps_x.data(), in.kw, s.taps_y.data(), in.kh, in.shift, s.divisor, in.op,
                          in.border)) != VF_OK)
        return rc;
      s.kw = in.kw, s.kh = in.kh, s.shift = in.shift, s.border = in.border;
    } else if (in.kind == VF_STEP_LEVEL) {
      // data: {mask, link, clip_lo, clip_hi} as int32; op: the rule
      const int32_t *d = static_cast<const int32_t *>(in.data);
      if (!d) return set_err(ctx, VF_E_INVALID, 0, "%s: the level step's data is NULL", at);
      if ((rc = check_level(ctx, at, in.op, d[0], d[1], d[2], d[3], channels)) != VF_OK) return rc;
      s.mask = d[0], s.link = d[1], s.clip_lo = d[2], s.clip_hi = d[3];
    } else if (in.kind == VF_STEP_CLAHE) {
      // data: {mask, clip_q8, tiles_x, tiles_y} as int32
      const int32_t *d = static_cast<const int32_t *>(in.data);
      if (!d) return set_err(ctx, VF_E_INVALID, 0, "%s: the CLAHE step's data is NULL", at);
      if ((rc = check_clahe(ctx, at, d[1], d[2], d[3], d[0], channels)) != VF_OK) return rc;
      s.mask = d[0], s.clip_q8 = d[1], s.tiles_x = d[2], s.tiles_y = d[3];
    } else if (in.kind == VF_STEP_WARP) {
      // data: six float64 (m), then {mode, interp, value B, G, R, 0} as int32; border: a VF_BORDER_*
      if (!in.data) return set_err(ctx, VF_E_INVALID, 0, "%s: the warp step's data is NULL", at);
      WarpStepData d;
      std::memcpy(&d, in.data, sizeof d);  // host memory of any alignment
      if ((rc = check_warp(ctx, at, d.m, d.i[0], d.i[1], in.border, d.i + 2, channels)) != VF_OK) return rc;
      std::memcpy(s.warp.m, d.m, sizeof d.m);
      s.warp.mode = d.i[0], s.warp.interp = d.i[1], s.border = in.border;
      for (int c = 0; c < 3; ++c) s.warp.value[c] = (uint8_t)d.i[2 + c];
    } else if (in.kind == VF_STEP_RESIZE) {
      // data: two float64 {fx, fy}, then {dw, dh, interp, 0} as int32
      if (!in.data) return set_err(ctx, VF_E_INVALID, 0, "%s: the resize step's data is NULL", at);
      ResizeStepData d;
      std::memcpy(&d, in.data, sizeof d);  // host memory of any alignment
      if ((rc = check_resize(ctx, at, d.i[0], d.i[1], d.f[0], d.f[1], d.i[2], channels)) != VF_OK) return rc;
      s.resize.fx = d.f[0], s.resize.fy = d.f[1];
      s.resize.dw = d.i[0], s.resize.dh = d.i[1], s.resize.interp = d.i[2];
    } else if (in.kind != VF_STEP_BINARY) {
      return set_err(ctx, VF_E_INVALID, 0, "%s: unknown kind %d", at, in.kind);
    }
    p.steps.push_back(std::move(s));
  }
  std::string why;
  if (!vf::chain::validate(p, channels, &why)) return set_err(ctx, VF_E_INVALID, 0, "%s: %s", fn, why.c_str());
  *out = vf::chain::fold(p);
  masks->assign(out->steps.size(), 0);
  for (size_t i = 0; i < out->steps.size(); ++i) {
    const vf::chain::Step &s = out->steps[i];
    if (s.kind == vf::chain::kRank) (*masks)[i] = vf::rank_mask(s.element.data(), s.kw, s.kh);
  }
  return VF_OK;
}

}  // namespace

VF_EXPORT int vf_binary_device(vf_ctx *ctx, const void *da, const void *db, void *ddst, size_t nbytes, int op,
                               void *stream) {
  VF_CHECK_CTX(ctx);
  if (op < VF_BIN_SUBTRACT || op > VF_BIN_MAX) return set_err(ctx, VF_E_INVALID, 0, "vf_binary_device: unknown op %d", op);
  if (nbytes == 0) return VF_OK;
  if (!da || !db || !ddst) return set_err(ctx, VF_E_INVALID, 0, "vf_binary_device: NULL buffer");
  if (overlaps_partially((const uint8_t *)da, (const uint8_t *)ddst, nbytes) ||
      overlaps_partially((const uint8_t *)db, (const uint8_t *)ddst, nbytes))
    return set_err(ctx, VF_E_INVALID, 0, "vf_binary_device: dst partially overlaps an operand");
  VF_HIP(ctx, hipSetDevice(ctx->device));
  VF_HIP(ctx, vf::launch_binary(da, db, ddst, nbytes, op, ctx->cfg, (hipStream_t)stream));
  return VF_OK;
}

VF_EXPORT int vf_chain_frames_host(vf_ctx *ctx, const uint8_t *const *srcs, uint8_t *const *dsts, const int *widths,
                                   const int *heights, int n, int channels, const vf_step *steps, int nsteps) {
  VF_CHECK_CTX(ctx);
  return program_frames_host(ctx, "vf_chain_frames_host", srcs, dsts, widths, heights, n, channels, steps, nsteps);
}

VF_EXPORT int vf_chain_out_size(vf_ctx *ctx, const vf_step *steps, int nsteps, int channels, int width, int height,
                                int *out_w, int *out_h) {
  VF_CHECK_CTX(ctx);
  const char *fn = "vf_chain_out_size";
  if (!out_w || !out_h) return set_err(ctx, VF_E_INVALID, 0, "%s: NULL result", fn);
  vf::chain::Program prog;
  std::vector<uint64_t> masks;
  int rc = chain_program(ctx, fn, steps, nsteps, channels, &prog, &masks);
  if (rc != VF_OK) return rc;
  *out_w = width, *out_h = height;
  if (width == 0 && height == 0) return VF_OK;  // the empty frame stays empty
  if ((rc = check_frame_shape(ctx, fn, width, height, channels)) != VF_OK) return rc;
  if (!vf::chain::has_resize(prog)) return VF_OK;
  std::vector<vf::chain::Size> sizes;
  std::string why;
  if (!vf::chain::value_sizes(prog, width, height, &sizes, &why)) return set_err(ctx, VF_E_INVALID, 0, "%s: %s", fn, why.c_str());
  *out_w = sizes.back().w, *out_h = sizes.back().h;
  return VF_OK;
}

// ---- memory helpers ------------------------------------------------------------------------

VF_EXPORT int vf_alloc_device(vf_ctx *ctx, size_t nbytes, void **out) {
  VF_CHECK_CTX(ctx);
  if (!out) return set_err(ctx, VF_E_INVALID, 0, "vf_alloc_device: out is NULL");
  *out = nullptr;
  VF_HIP(ctx, hipSetDevice(ctx->device));
  hipError_t e = hipMalloc(out, nbytes ? nbytes : 1);
  if (e != hipSuccess)
    return set_err(ctx, VF_E_NOMEM, (int)e, "hipMalloc(%zu) failed: %s", nbytes, hipGetErrorString(e));
  return VF_OK;
}

VF_EXPORT int vf_free_device(vf_ctx *ctx, void *p) {
  VF_CHECK_CTX(ctx);
  if (!p) return VF_OK;
  VF_HIP(ctx, hipSetDevice(ctx->device));
  VF_HIP(ctx, hipFree(p));
  return VF_OK;
}

VF_EXPORT int vf_alloc_host(vf_ctx *ctx, size_t nbytes, void **out) {
  VF_CHECK_CTX(ctx);
  if (!out) return set_err(ctx, VF_E_INVALID, 0, "vf_alloc_host: out is NULL");
  *out = nullptr;
  VF_HIP(ctx, hipSetDevice(ctx->device));
  hipError_t e = vf::numa_pinned_alloc(out, nbytes ? nbytes : 1, vf::device_numa_node(ctx->device));
  if (e != hipSuccess)
    return set_err(ctx, VF_E_NOMEM, (int)e, "pinned allocation of %zu bytes failed: %s", nbytes, hipGetErrorString(e));
  ctx->engine->note_pinned(*out, nbytes ? nbytes : 1);
  return VF_OK;
}

VF_EXPORT int vf_free_host(vf_ctx *ctx, void *p) {
  VF_CHECK_CTX(ctx);
  if (!p) return VF_OK;
  ctx->engine->drain();  // a queued job may still read or write it
  ctx->engine->forget_pinned(p);
  VF_HIP(ctx, vf::numa_pinned_free(p));
  return VF_OK;
}

VF_EXPORT int vf_host_register(vf_ctx *ctx, void *p, size_t nbytes) {
  VF_CHECK_CTX(ctx);
  if (!p || !nbytes) return set_err(ctx, VF_E_INVALID, 0, "vf_host_register: empty range");
  VF_HIP(ctx, hipSetDevice(ctx->device));
  VF_HIP(ctx, hipHostRegister(p, nbytes, hipHostRegisterMapped));
  ctx->engine->note_pinned(p, nbytes);
  return VF_OK;
}

VF_EXPORT int vf_host_unregister(vf_ctx *ctx, void *p) {
  VF_CHECK_CTX(ctx);
  if (!p) return VF_OK;
  ctx->engine->drain();
  ctx->engine->forget_pinned(p);
  VF_HIP(ctx, hipHostUnregister(p));
  return VF_OK;
}

VF_EXPORT int vf_upload(vf_ctx *ctx, void *ddst, const void *hsrc, size_t nbytes, void *stream) {
  VF_CHECK_CTX(ctx);
  if (!nbytes) return VF_OK;
  if (!ddst || !hsrc) return set_err(ctx, VF_E_INVALID, 0, "vf_upload: NULL buffer");
  VF_HIP(ctx, hipSetDevice(ctx->device));
  VF_HIP(ctx, hipMemcpyAsync(ddst, hsrc, nbytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  return VF_OK;
}

VF_EXPORT int vf_download(vf_ctx *ctx, void *hdst, const void *dsrc, size_t nbytes, void *stream) {
  VF_CHECK_CTX(ctx);
  if (!nbytes) return VF_OK;
  if (!hdst || !dsrc) return set_err(ctx, VF_E_INVALID, 0, "vf_download: NULL buffer");
  VF_HIP(ctx, hipSetDevice(ctx->device));
  VF_HIP(ctx, hipMemcpyAsync(hdst, dsrc, nbytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
  return VF_OK;
}

VF_EXPORT int vf_memset_device(vf_ctx *ctx, void *d, int value, size_t nbytes, void *stream) {
  VF_CHECK_CTX(ctx);
  if (!nbytes) return VF_OK;
  if (!d) return set_err(ctx, VF_E_INVALID, 0, "vf_memset_device: NULL buffer");
  VF_HIP(ctx, hipSetDevice(ctx->device));
  VF_HIP(ctx, hipMemsetAsync(d, value, nbytes, (hipStream_t)stream));
  return VF_OK;
}

VF_EXPORT int vf_sync(vf_ctx *ctx, void *stream) {
  VF_CHECK_CTX(ctx);
  VF_HIP(ctx, hipSetDevice(ctx->device));
  if (stream) {
    VF_HIP(ctx, hipStreamSynchronize((hipStream_t)stream));
  } else {
    ctx->engine->drain();
    VF_HIP(ctx, hipDeviceSynchronize());
  }
  return VF_OK;
}

// ---- timing ----------------------------------------------------------------------------

VF_EXPORT int vf_elapsed_ms(const vf_ctx *ctx, float *out_ms) {
  if (!ctx || !out_ms) return set_err(nullptr, VF_E_INVALID, 0, "vf_elapsed_ms: NULL argument");
  *out_ms = ctx->last_kernel_ms;
  return VF_OK;
}

VF_EXPORT int vf_last_timeline(const vf_ctx *ctx, float *out4, size_t *chunk_bytes, int max_chunks,
                               int *n_chunks) {
  if (!ctx || !n_chunks) return set_err(nullptr, VF_E_INVALID, 0, "vf_last_timeline: NULL argument");
  const int n = (int)ctx->timeline.size();
  *n_chunks = n;
  for (int i = 0; i < n && i < max_chunks; ++i) {
    const vf::ChunkTime &t = ctx->timeline[(size_t)i];
    if (out4) {
      out4[4 * i + 0] = t.h2d_start;
      out4[4 * i + 1] = t.kernel_start;
      out4[4 * i + 2] = t.kernel_end;
      out4[4 * i + 3] = t.d2h_end;
    }
    if (chunk_bytes) chunk_bytes[i] = t.bytes;
  }
  return VF_OK;
}

VF_EXPORT int vf_bench_device_ring(vf_ctx *ctx, void *const *srcs, void *const *dsts, int nbuf,
                                   size_t nbytes, int steps, void *stream, float *per_launch_ms,
                                   float *region_ms) {
  VF_CHECK_CTX(ctx);
  if (!srcs || !dsts || nbuf < 1 || steps < 0)
    return set_err(ctx, VF_E_INVALID, 0, "vf_bench_device_ring: bad arguments");
  VF_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const bool each = per_launch_ms != nullptr;
  std::vector<hipEvent_t> ev(each ? 2 * (size_t)steps : 0, nullptr);
  int rc = VF_OK;
  for (auto &e : ev) {
    hipError_t h = hipEventCreate(&e);
    if (h != hipSuccess) { rc = fail_hip(ctx, h, "hipEventCreate", __LINE__); break; }
  }
  // the region pair is the context's, created by the first call (the warm-up): a timed call
  // then only records, launches and synchronises
  for (hipEvent_t &e : ctx->bench_ev) {
    if (rc != VF_OK || e) continue;
    hipError_t h = hipEventCreate(&e);
    if (h != hipSuccess) rc = fail_hip(ctx, h, "hipEventCreate", __LINE__);
  }
  hipEvent_t r0 = ctx->bench_ev[0], r1 = ctx->bench_ev[1];
  if (rc == VF_OK) {
    hipError_t h = hipEventRecord(r0, st);
    if (h != hipSuccess) rc = fail_hip(ctx, h, "hipEventRecord", __LINE__);
  }
  for (int s = 0; s < steps && rc == VF_OK; ++s) {
    hipError_t h = each ? hipEventRecord(ev[2 * s], st) : hipSuccess;
    if (h == hipSuccess) h = vf::launch_invert(srcs[s % nbuf], dsts[s % nbuf], nbytes, ctx->cfg, st);
    if (h == hipSuccess && each) h = hipEventRecord(ev[2 * s + 1], st);
    if (h != hipSuccess) rc = fail_hip(ctx, h, "bench launch", __LINE__);
  }
  if (rc == VF_OK) {
    hipError_t h = hipEventRecord(r1, st);
    if (h == hipSuccess) h = hipStreamSynchronize(st);
    if (h != hipSuccess) rc = fail_hip(ctx, h, "hipStreamSynchronize", __LINE__);
  }
  for (int s = 0; s < steps && rc == VF_OK && each; ++s) {
    float ms = 0.f;
    hipError_t h = hipEventElapsedTime(&ms, ev[2 * s], ev[2 * s + 1]);
    if (h != hipSuccess) { rc = fail_hip(ctx, h, "hipEventElapsedTime", __LINE__); break; }
    per_launch_ms[s] = ms;
  }
  if (rc == VF_OK && region_ms) {
    float ms = 0.f;
    hipError_t h = hipEventElapsedTime(&ms, r0, r1);
    if (h != hipSuccess) rc = fail_hip(ctx, h, "hipEventElapsedTime", __LINE__);
    *region_ms = ms;
  }
  for (auto &e : ev)
    if (e) (void)hipEventDestroy(e);
  return rc;
}

// ---- JPEG (inverter.py:32 / :41 / :44 in the default use_jpeg=True mode) --------------------

namespace {

// A free codec, or a new one while the context has fewer than `most` (ctx->jpeg_mu held); nullptr
// when neither, or out of host memory.
vf::jpeg::Codec *take_codec(vf_ctx *ctx, size_t most) {
  vf::jpeg::Codec *c = nullptr;
  if (!ctx->jpeg_free.empty()) {
    c = ctx->jpeg_free.back();
    ctx->jpeg_free.pop_back();
  } else if (ctx->jpeg_all.size() < most) {
    static const bool gated = env_size("VF_JPEG_GATE", 0) != 0;
    c = new (std::nothrow) vf::jpeg::Codec(ctx->device, gated ? &ctx->jpeg_gate : nullptr);
    if (c) ctx->jpeg_all.push_back(c);
  }
  if (c) c->set_max_pixels(ctx->jpeg_max_pixels.load());
  return c;
}

// A codec leased to one call for its duration (blocks while all codecs are busy).
class CodecLease {
 public:
  explicit CodecLease(vf_ctx *ctx) : ctx_(ctx) {
    static const size_t kMax = std::max<size_t>(1, env_size("VF_JPEG_CODECS", 2));
    std::unique_lock<std::mutex> lk(ctx->jpeg_mu);
    ctx->jpeg_cv.wait(lk, [&] { return !ctx->jpeg_free.empty() || ctx->jpeg_all.size() < kMax; });
    c_ = take_codec(ctx, kMax);
  }
  ~CodecLease() {
    if (!c_) return;
    c_->quiesce();  // a failed call may have left work queued (no-op after a success)
    {
      std::lock_guard<std::mutex> lk(ctx_->jpeg_mu);
      ctx_->jpeg_free.push_back(c_);
    }
    ctx_->jpeg_cv.notify_one();
  }
  CodecLease(const CodecLease &) = delete;
  CodecLease &operator=(const CodecLease &) = delete;
  vf::jpeg::Codec *get() const { return c_; }

 private:
  vf_ctx *ctx_;
  vf::jpeg::Codec *c_ = nullptr;
};

// A codec for an asynchronous batch: never blocks (the caller thread may be the one that would
// fetch the batches holding the others); a new codec when none is free, up to kMaxJpegJobs.
constexpr size_t kMaxJpegJobs = 8;
vf::jpeg::Codec *lease_nowait(vf_ctx *ctx) {
  std::lock_guard<std::mutex> lk(ctx->jpeg_mu);
  return take_codec(ctx, kMaxJpegJobs);
}

void give_back(vf_ctx *ctx, vf::jpeg::Codec *c) {
  {
    std::lock_guard<std::mutex> lk(ctx->jpeg_mu);
    ctx->jpeg_free.push_back(c);
  }
  ctx->jpeg_cv.notify_one();
}

vf::jpeg::Codec *job_codec(vf_ctx *ctx, uint64_t ticket) {
  std::lock_guard<std::mutex> lk(ctx->jpeg_mu);
  auto it = ctx->jpeg_jobs.find(ticket);
  return it == ctx->jpeg_jobs.end() ? nullptr : it->second;
}

void end_job(vf_ctx *ctx, uint64_t ticket) {
  vf::jpeg::Codec *c = nullptr;
  {
    std::lock_guard<std::mutex> lk(ctx->jpeg_mu);
    auto it = ctx->jpeg_jobs.find(ticket);
    if (it == ctx->jpeg_jobs.end()) return;
    c = it->second;
    ctx->jpeg_jobs.erase(it);
  }
  c->quiesce();
  give_back(ctx, c);
}

int jpeg_codec(vf_ctx *ctx, const CodecLease &lease, vf::jpeg::Codec **out) {
  if (!lease.get()) return set_err(ctx, VF_E_NOMEM, 0, "JPEG codec: out of host memory");
  *out = lease.get();
  return VF_OK;
}

int jpeg_status(vf_ctx *ctx, int rc, const std::string &msg) {
  if (rc == VF_OK) return VF_OK;
  return set_err(ctx, rc, 0, "%s", msg.c_str());
}

}  // namespace

VF_EXPORT int vf_jpeg_header(const uint8_t *jpeg, size_t size, int *width, int *height, int *subsamp,
                             int *colorspace) {
  if (!width || !height || !subsamp || !colorspace)
    return set_err(nullptr, VF_E_INVALID, 0, "vf_jpeg_header: NULL output pointer");
  std::string err;
  const int rc = vf::jpeg::header_info(jpeg, size, width, height, subsamp, colorspace, &err);
  return rc == VF_OK ? VF_OK : set_err(nullptr, rc, 0, "vf_jpeg_header: %s", err.c_str());
}

VF_EXPORT int vf_jpeg_set_max_pixels(vf_ctx *ctx, uint64_t max_pixels) {
  if (!ctx) return set_err(nullptr, VF_E_INVALID, 0, "vf_jpeg_set_max_pixels: NULL context");
  ctx->jpeg_max_pixels.store(max_pixels ? max_pixels : vf::jpeg::kDefaultMaxPixels);
  return VF_OK;
}

VF_EXPORT size_t vf_jpeg_buffer_size(int width, int height, int subsamp) {
  return vf::jpeg::buffer_size(width, height, subsamp);
}

VF_EXPORT int vf_jpeg_encode(vf_ctx *ctx, const uint8_t *const *imgs, const int *widths, const int *heights, int n,
                             int pixel_format, int quality, int subsamp, int flags, uint8_t *const *outs,
                             const size_t *caps, size_t *sizes) {
  VF_CHECK_CTX(ctx);
  if (n < 0 || (n > 0 && (!imgs || !widths || !heights || !outs || !caps || !sizes)))
    return set_err(ctx, VF_E_INVALID, 0, "vf_jpeg_encode: bad arguments");
  if (n > 65535) return set_err(ctx, VF_E_INVALID, 0, "vf_jpeg_encode: at most 65535 frames per call");
  CodecLease lease(ctx);
  vf::jpeg::Codec *c = nullptr;
  int rc = jpeg_codec(ctx, lease, &c);
  if (rc) return rc;
  std::string err;
  rc = c->encode(imgs, widths, heights, n, pixel_format, quality, subsamp, flags, outs, caps, sizes, &err);
  return jpeg_status(ctx, rc, "vf_jpeg_encode: " + err);
}

VF_EXPORT int vf_jpeg_decode(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                             int pixel_format, int flags, uint8_t *const *outs, const size_t *caps) {
  VF_CHECK_CTX(ctx);
  if (n < 0 || (n > 0 && (!jpegs || !jpeg_sizes || !outs || !caps)))
    return set_err(ctx, VF_E_INVALID, 0, "vf_jpeg_decode: bad arguments");
  if (n > 65535) return set_err(ctx, VF_E_INVALID, 0, "vf_jpeg_decode: at most 65535 frames per call");
  CodecLease lease(ctx);
  vf::jpeg::Codec *c = nullptr;
  int rc = jpeg_codec(ctx, lease, &c);
  if (rc) return rc;
  std::string err;
  rc = c->decode(jpegs, jpeg_sizes, n, pixel_format, flags, outs, caps, &err);
  return jpeg_status(ctx, rc, "vf_jpeg_decode: " + err);
}

namespace {

using vf::jpeg::Filter;

// decode -> filter -> encode, for every vf_jpeg_{invert,lut,conv,rank}
int jpeg_filter(vf_ctx *ctx, const char *fn, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n, int quality,
                int subsamp, int flags, uint8_t *const *outs, const size_t *caps, size_t *sizes, const Filter &filt) {
  if (n < 0 || (n > 0 && (!jpegs || !jpeg_sizes || !outs || !caps || !sizes)))
    return set_err(ctx, VF_E_INVALID, 0, "%s: bad arguments", fn);
  if (n > 65535) return set_err(ctx, VF_E_INVALID, 0, "%s: at most 65535 frames per call", fn);
  CodecLease lease(ctx);
  vf::jpeg::Codec *c = nullptr;
  int rc = jpeg_codec(ctx, lease, &c);
  if (rc) return rc;
  std::string err;
  rc = c->invert(jpegs, jpeg_sizes, n, quality, subsamp, flags, outs, caps, sizes, filt, &err);
  return jpeg_status(ctx, rc, std::string(fn) + ": " + err);
}

int jpeg_filter_submit(vf_ctx *ctx, const char *fn, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                       int quality, int subsamp, int flags, uint64_t *ticket, const Filter &filt) {
  if (!ticket || n <= 0 || n > 65535 || !jpegs || !jpeg_sizes)
    return set_err(ctx, VF_E_INVALID, 0, "%s: bad arguments", fn);
  *ticket = 0;
  vf::jpeg::Codec *c = lease_nowait(ctx);
  if (!c)
    return set_err(ctx, VF_E_INVALID, 0, "%s: %zu batches already in flight; fetch one first", fn, kMaxJpegJobs);
  std::string err;
  const int rc = c->submit_invert(jpegs, jpeg_sizes, n, quality, subsamp, flags, filt, &err);
  if (rc != VF_OK) {
    c->quiesce();  // a submit that failed after queueing work must not hand the codec on mid-flight
    give_back(ctx, c);
    return jpeg_status(ctx, rc, std::string(fn) + ": " + err);
  }
  std::lock_guard<std::mutex> lk(ctx->jpeg_mu);
  *ticket = ctx->jpeg_next_ticket++;
  ctx->jpeg_jobs[*ticket] = c;
  return VF_OK;
}

int jpeg_filter_bench(vf_ctx *ctx, const char *fn, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                      int quality, int subsamp, int flags, int iters, float *ms, float *stage_ms, const Filter &filt) {
  if (n <= 0 || n > 65535 || !jpegs || !jpeg_sizes || !ms || iters <= 0)
    return set_err(ctx, VF_E_INVALID, 0, "%s: bad arguments", fn);
  CodecLease lease(ctx);
  vf::jpeg::Codec *c = nullptr;
  int rc = jpeg_codec(ctx, lease, &c);
  if (rc) return rc;
  std::string err;
  rc = c->bench_invert(jpegs, jpeg_sizes, n, quality, subsamp, flags, iters, filt, ms, stage_ms, &err);
  return jpeg_status(ctx, rc, std::string(fn) + ": " + err);
}

// The builders of a batch's filter from an entry point's arguments, checked first (fn: its
// name, for the message).  The inversion is Filter{}.
int table_filter(vf_ctx *ctx, const char *fn, const uint8_t *table, int channels, Filter *out) {
  const int rc = check_table(ctx, fn, table, channels);
  if (rc != VF_OK) return rc;
  out->kind = Filter::kTable;
  uint8_t *t = reinterpret_cast<uint8_t *>(out->lut.w);  // a one-channel table serves all three
  for (int c = 0; c < 3; ++c) std::memcpy(t + 256 * c, table + (channels == 3 ? 256 * c : 0), 256);
  return VF_OK;
}

// A program as a batch's filter.  One that folds to a single table runs as that table, in the fused
// colour stage; anything else is Filter::kChain, its plan built here once and shared by the codec's
// copy.  The decoded frames have three channels.
int chain_filter(vf_ctx *ctx, const char *fn, const vf_step *steps, int nsteps, Filter *out) {
  auto spec = std::make_shared<vf::jpeg::ChainSpec>();
  const int rc = chain_program(ctx, fn, steps, nsteps, 3, &spec->prog, &spec->masks);
  if (rc != VF_OK) return rc;
  if (vf::chain::single_kind(spec->prog) == vf::chain::kTable)
    return table_filter(ctx, fn, spec->prog.steps[0].table.data(), spec->prog.steps[0].channels, out);
  // under a resize step the decoded frames keep buffer 0 to themselves (vf_jpeg_host.hip run_filter_encode)
  spec->bufs = vf::chain::assign_buffers(spec->prog, vf::chain::has_resize(spec->prog));
  out->kind = Filter::kChain;
  out->chain = std::move(spec);
  return VF_OK;
}

// A convolution or a rank filter is a program of one step.
int conv_filter(vf_ctx *ctx, const char *fn, const int16_t *weights, int kw, int kh, int shift, int border,
                Filter *out) {
  const int rc = check_kernel(ctx, fn, weights, kw, kh, shift, border);
  if (rc != VF_OK) return rc;
  const vf_step step{VF_STEP_CONV, 0, 0, 0, weights, kw, kh, shift, border, 0};
  return chain_filter(ctx, fn, &step, 1, out);
}

int rank_filter(vf_ctx *ctx, const char *fn, int op, const uint8_t *element, int kw, int kh, int border, Filter *out) {
  uint64_t mask = 0;
  const int rc = check_rank(ctx, fn, op, element, kw, kh, border, &mask);
  if (rc != VF_OK) return rc;
  const vf_step step{VF_STEP_RANK, 0, 0, op, element, kw, kh, 0, border, 0};
  return chain_filter(ctx, fn, &step, 1, out);
}

int mix_filter(vf_ctx *ctx, const char *fn, const int32_t *matrix, int shift, int rounding, Filter *out) {
  const int rc = check_mix(ctx, fn, matrix, shift, rounding);
  if (rc != VF_OK) return rc;
  const vf_step step{VF_STEP_MIX, 0, 0, rounding, matrix, 0, 0, shift, 0, 0};
  return chain_filter(ctx, fn, &step, 1, out);
}

int sep_filter(vf_ctx *ctx, const char *fn, const int16_t *kx, int kw, const int16_t *ky, int kh, int shift, int divisor,
               int rounding, int border, Filter *out) {
  const int rc = check_sep(ctx, fn, kx, kw, ky, kh, shift, divisor, rounding, border);
  if (rc != VF_OK) return rc;
  const std::vector<int32_t> data = sep_step_data(kx, kw, ky, kh, divisor);
  const vf_step step{VF_STEP_SEP, 0, 0, rounding, data.data(), kw, kh, shift, border, 0};
  return chain_filter(ctx, fn, &step, 1, out);
}

// The decoded frames are 3-channel BGR, grayscale inputs included.
int level_filter(vf_ctx *ctx, const char *fn, int rule, int mask, int link, int clip_lo, int clip_hi, Filter *out) {
  const int rc = check_level(ctx, fn, rule, mask, link, clip_lo, clip_hi, 3);
  if (rc != VF_OK) return rc;
  const int32_t data[4] = {mask, link, clip_lo, clip_hi};
  const vf_step step{VF_STEP_LEVEL, 0, 0, rule, data, 0, 0, 0, 0, 0};
  return chain_filter(ctx, fn, &step, 1, out);
}

// The decoded frames are 3-channel BGR, grayscale inputs included.
int clahe_filter(vf_ctx *ctx, const char *fn, int clip_q8, int tiles_x, int tiles_y, int mask, Filter *out) {
  const int rc = check_clahe(ctx, fn, clip_q8, tiles_x, tiles_y, mask, 3);
  if (rc != VF_OK) return rc;
  const int32_t data[4] = {mask, clip_q8, tiles_x, tiles_y};
  const vf_step step{VF_STEP_CLAHE, 0, 0, 0, data, 0, 0, 0, 0, 0};
  return chain_filter(ctx, fn, &step, 1, out);
}

// The decoded frames are 3-channel BGR, grayscale inputs included; the encoder takes the result's size.
int resize_filter(vf_ctx *ctx, const char *fn, int dw, int dh, double fx, double fy, int interp, Filter *out) {
  const int rc = check_resize(ctx, fn, dw, dh, fx, fy, interp, 3);
  if (rc != VF_OK) return rc;
  const ResizeStepData data = resize_step_data(dw, dh, fx, fy, interp);
  const vf_step step{VF_STEP_RESIZE, 0, 0, 0, &data, 0, 0, 0, 0, 0};
  return chain_filter(ctx, fn, &step, 1, out);
}

// The decoded frames are 3-channel BGR, grayscale inputs included.
int warp_filter(vf_ctx *ctx, const char *fn, const double *m, int mode, int interp, int border, const int *value,
                Filter *out) {
  const int rc = check_warp(ctx, fn, m, mode, interp, border, value, 3);
  if (rc != VF_OK) return rc;
  const WarpStepData data = warp_step_data(m, mode, interp, value);
  const vf_step step{VF_STEP_WARP, 0, 0, 0, &data, 0, 0, 0, border, 0};
  return chain_filter(ctx, fn, &step, 1, out);
}

}  // namespace

VF_EXPORT int vf_jpeg_invert(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n, int quality,
                             int subsamp, int flags, uint8_t *const *outs, const size_t *caps, size_t *sizes) {
  VF_CHECK_CTX(ctx);
  return jpeg_filter(ctx, "vf_jpeg_invert", jpegs, jpeg_sizes, n, quality, subsamp, flags, outs, caps, sizes, Filter{});
}

VF_EXPORT int vf_jpeg_invert_submit(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                                    int quality, int subsamp, int flags, uint64_t *ticket) {
  VF_CHECK_CTX(ctx);
  return jpeg_filter_submit(ctx, "vf_jpeg_invert_submit", jpegs, jpeg_sizes, n, quality, subsamp, flags, ticket,
                            Filter{});
}

VF_EXPORT int vf_jpeg_lut(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                          const uint8_t *table, int channels, int quality, int subsamp, int flags,
                          uint8_t *const *outs, const size_t *caps, size_t *sizes) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = table_filter(ctx, "vf_jpeg_lut", table, channels, &filter)) return rc;
  return jpeg_filter(ctx, "vf_jpeg_lut", jpegs, jpeg_sizes, n, quality, subsamp, flags, outs, caps, sizes, filter);
}

VF_EXPORT int vf_jpeg_lut_submit(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                                 const uint8_t *table, int channels, int quality, int subsamp, int flags,
                                 uint64_t *ticket) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = table_filter(ctx, "vf_jpeg_lut_submit", table, channels, &filter)) return rc;
  return jpeg_filter_submit(ctx, "vf_jpeg_lut_submit", jpegs, jpeg_sizes, n, quality, subsamp, flags, ticket, filter);
}

VF_EXPORT int vf_jpeg_invert_query(vf_ctx *ctx, uint64_t ticket, int *done) {
  VF_CHECK_CTX(ctx);
  vf::jpeg::Codec *c = job_codec(ctx, ticket);
  if (!c || !done) return set_err(ctx, VF_E_INVALID, 0, "vf_jpeg_invert_query: unknown ticket %llu",
                                  (unsigned long long)ticket);
  *done = c->done_invert() ? 1 : 0;
  return VF_OK;
}

VF_EXPORT int vf_jpeg_invert_wait(vf_ctx *ctx, uint64_t ticket, size_t *total) {
  VF_CHECK_CTX(ctx);
  vf::jpeg::Codec *c = job_codec(ctx, ticket);
  if (!c || !total) return set_err(ctx, VF_E_INVALID, 0, "vf_jpeg_invert_wait: unknown ticket %llu",
                                   (unsigned long long)ticket);
  std::string err;
  const int rc = c->wait_invert(total, &err);
  if (rc != VF_OK) end_job(ctx, ticket);  // a failed batch is over: its codec is free again
  return jpeg_status(ctx, rc, "vf_jpeg_invert_wait: " + err);
}

VF_EXPORT int vf_jpeg_invert_fetch(vf_ctx *ctx, uint64_t ticket, uint8_t *out, size_t cap, size_t *sizes,
                                   size_t *offsets) {
  VF_CHECK_CTX(ctx);
  vf::jpeg::Codec *c = job_codec(ctx, ticket);
  if (!c) return set_err(ctx, VF_E_INVALID, 0, "vf_jpeg_invert_fetch: unknown ticket %llu", (unsigned long long)ticket);
  std::string err;
  int rc = VF_OK;
  if (!c->waited()) {  // fetch without wait: wait here (out == NULL just releases the batch)
    size_t total = 0;
    rc = c->wait_invert(&total, &err);
  }
  if (rc == VF_OK) rc = c->fetch_invert(out, cap, sizes, offsets, &err);
  if (rc == VF_E_INVALID && out && cap) return jpeg_status(ctx, rc, "vf_jpeg_invert_fetch: " + err);  // retry with room
  end_job(ctx, ticket);
  return jpeg_status(ctx, rc, "vf_jpeg_invert_fetch: " + err);
}

VF_EXPORT int vf_jpeg_invert_scatter(vf_ctx *ctx, uint64_t ticket, uint8_t *const *outs, const size_t *caps,
                                     size_t *sizes, int *placed) {
  VF_CHECK_CTX(ctx);
  vf::jpeg::Codec *c = job_codec(ctx, ticket);
  if (!c || !outs || !caps || !sizes || !placed)
    return set_err(ctx, VF_E_INVALID, 0, "vf_jpeg_invert_scatter: unknown ticket %llu or NULL argument",
                   (unsigned long long)ticket);
  if (!c->waited()) return set_err(ctx, VF_E_INVALID, 0, "vf_jpeg_invert_scatter: call vf_jpeg_invert_wait first");
  return jpeg_status(ctx, c->scatter_invert(outs, caps, sizes, placed), "vf_jpeg_invert_scatter");
}

VF_EXPORT int vf_jpeg_bench_invert(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                                   int quality, int subsamp, int flags, int iters, float *ms, float *stage_ms) {
  VF_CHECK_CTX(ctx);
  return jpeg_filter_bench(ctx, "vf_jpeg_bench_invert", jpegs, jpeg_sizes, n, quality, subsamp, flags, iters, ms,
                           stage_ms, Filter{});
}

VF_EXPORT int vf_jpeg_bench_lut(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                                const uint8_t *table, int channels, int quality, int subsamp, int flags, int iters,
                                float *ms, float *stage_ms) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = table_filter(ctx, "vf_jpeg_bench_lut", table, channels, &filter)) return rc;
  return jpeg_filter_bench(ctx, "vf_jpeg_bench_lut", jpegs, jpeg_sizes, n, quality, subsamp, flags, iters, ms, stage_ms,
                           filter);
}

VF_EXPORT int vf_jpeg_conv(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                           const int16_t *weights, int kw, int kh, int shift, int border, int quality, int subsamp,
                           int flags, uint8_t *const *outs, const size_t *caps, size_t *sizes) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = conv_filter(ctx, "vf_jpeg_conv", weights, kw, kh, shift, border, &filter)) return rc;
  return jpeg_filter(ctx, "vf_jpeg_conv", jpegs, jpeg_sizes, n, quality, subsamp, flags, outs, caps, sizes, filter);
}

VF_EXPORT int vf_jpeg_conv_submit(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                                  const int16_t *weights, int kw, int kh, int shift, int border, int quality,
                                  int subsamp, int flags, uint64_t *ticket) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = conv_filter(ctx, "vf_jpeg_conv_submit", weights, kw, kh, shift, border, &filter)) return rc;
  return jpeg_filter_submit(ctx, "vf_jpeg_conv_submit", jpegs, jpeg_sizes, n, quality, subsamp, flags, ticket, filter);
}

VF_EXPORT int vf_jpeg_bench_conv(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                                 const int16_t *weights, int kw, int kh, int shift, int border, int quality,
                                 int subsamp, int flags, int iters, float *ms, float *stage_ms) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = conv_filter(ctx, "vf_jpeg_bench_conv", weights, kw, kh, shift, border, &filter)) return rc;
  return jpeg_filter_bench(ctx, "vf_jpeg_bench_conv", jpegs, jpeg_sizes, n, quality, subsamp, flags, iters, ms,
                           stage_ms, filter);
}

VF_EXPORT int vf_jpeg_rank(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n, int op,
                           const uint8_t *element, int kw, int kh, int border, int quality, int subsamp, int flags,
                           uint8_t *const *outs, const size_t *caps, size_t *sizes) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = rank_filter(ctx, "vf_jpeg_rank", op, element, kw, kh, border, &filter)) return rc;
  return jpeg_filter(ctx, "vf_jpeg_rank", jpegs, jpeg_sizes, n, quality, subsamp, flags, outs, caps, sizes, filter);
}

VF_EXPORT int vf_jpeg_rank_submit(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n, int op,
                                  const uint8_t *element, int kw, int kh, int border, int quality, int subsamp,
                                  int flags, uint64_t *ticket) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = rank_filter(ctx, "vf_jpeg_rank_submit", op, element, kw, kh, border, &filter)) return rc;
  return jpeg_filter_submit(ctx, "vf_jpeg_rank_submit", jpegs, jpeg_sizes, n, quality, subsamp, flags, ticket, filter);
}

VF_EXPORT int vf_jpeg_bench_rank(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n, int op,
                                 const uint8_t *element, int kw, int kh, int border, int quality, int subsamp,
                                 int flags, int iters, float *ms, float *stage_ms) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = rank_filter(ctx, "vf_jpeg_bench_rank", op, element, kw, kh, border, &filter)) return rc;
  return jpeg_filter_bench(ctx, "vf_jpeg_bench_rank", jpegs, jpeg_sizes, n, quality, subsamp, flags, iters, ms,
                           stage_ms, filter);
}

// ---- JPEG with a colour matrix in place of the inversion --------------------------------------------

VF_EXPORT int vf_jpeg_mix(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                          const int32_t *matrix, int shift, int rounding, int quality, int subsamp, int flags,
                          uint8_t *const *outs, const size_t *caps, size_t *sizes) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = mix_filter(ctx, "vf_jpeg_mix", matrix, shift, rounding, &filter)) return rc;
  return jpeg_filter(ctx, "vf_jpeg_mix", jpegs, jpeg_sizes, n, quality, subsamp, flags, outs, caps, sizes, filter);
}

VF_EXPORT int vf_jpeg_mix_submit(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                                 const int32_t *matrix, int shift, int rounding, int quality, int subsamp, int flags,
                                 uint64_t *ticket) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = mix_filter(ctx, "vf_jpeg_mix_submit", matrix, shift, rounding, &filter)) return rc;
  return jpeg_filter_submit(ctx, "vf_jpeg_mix_submit", jpegs, jpeg_sizes, n, quality, subsamp, flags, ticket, filter);
}

VF_EXPORT int vf_jpeg_bench_mix(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                                const int32_t *matrix, int shift, int rounding, int quality, int subsamp, int flags,
                                int iters, float *ms, float *stage_ms) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = mix_filter(ctx, "vf_jpeg_bench_mix", matrix, shift, rounding, &filter)) return rc;
  return jpeg_filter_bench(ctx, "vf_jpeg_bench_mix", jpegs, jpeg_sizes, n, quality, subsamp, flags, iters, ms, stage_ms,
                           filter);
}

// ---- JPEG with a separable filter in place of the inversion ------------------------------------------

VF_EXPORT int vf_jpeg_sep(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n, const int16_t *kx,
                          int kw, const int16_t *ky, int kh, int shift, int divisor, int rounding, int border,
                          int quality, int subsamp, int flags, uint8_t *const *outs, const size_t *caps, size_t *sizes) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = sep_filter(ctx, "vf_jpeg_sep", kx, kw, ky, kh, shift, divisor, rounding, border, &filter)) return rc;
  return jpeg_filter(ctx, "vf_jpeg_sep", jpegs, jpeg_sizes, n, quality, subsamp, flags, outs, caps, sizes, filter);
}

VF_EXPORT int vf_jpeg_sep_submit(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                                 const int16_t *kx, int kw, const int16_t *ky, int kh, int shift, int divisor,
                                 int rounding, int border, int quality, int subsamp, int flags, uint64_t *ticket) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = sep_filter(ctx, "vf_jpeg_sep_submit", kx, kw, ky, kh, shift, divisor, rounding, border, &filter))
    return rc;
  return jpeg_filter_submit(ctx, "vf_jpeg_sep_submit", jpegs, jpeg_sizes, n, quality, subsamp, flags, ticket, filter);
}

VF_EXPORT int vf_jpeg_bench_sep(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                                const int16_t *kx, int kw, const int16_t *ky, int kh, int shift, int divisor,
                                int rounding, int border, int quality, int subsamp, int flags, int iters, float *ms,
                                float *stage_ms) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = sep_filter(ctx, "vf_jpeg_bench_sep", kx, kw, ky, kh, shift, divisor, rounding, border, &filter))
    return rc;
  return jpeg_filter_bench(ctx, "vf_jpeg_bench_sep", jpegs, jpeg_sizes, n, quality, subsamp, flags, iters, ms, stage_ms,
                           filter);
}

// ---- JPEG with the level filter in place of the inversion ---------------------------------------------

VF_EXPORT int vf_jpeg_level(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n, int rule, int mask,
                            int link, int clip_lo, int clip_hi, int quality, int subsamp, int flags, uint8_t *const *outs,
                            const size_t *caps, size_t *sizes) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = level_filter(ctx, "vf_jpeg_level", rule, mask, link, clip_lo, clip_hi, &filter)) return rc;
  return jpeg_filter(ctx, "vf_jpeg_level", jpegs, jpeg_sizes, n, quality, subsamp, flags, outs, caps, sizes, filter);
}

VF_EXPORT int vf_jpeg_level_submit(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n, int rule,
                                   int mask, int link, int clip_lo, int clip_hi, int quality, int subsamp, int flags,
                                   uint64_t *ticket) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = level_filter(ctx, "vf_jpeg_level_submit", rule, mask, link, clip_lo, clip_hi, &filter)) return rc;
  return jpeg_filter_submit(ctx, "vf_jpeg_level_submit", jpegs, jpeg_sizes, n, quality, subsamp, flags, ticket, filter);
}

VF_EXPORT int vf_jpeg_bench_level(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n, int rule,
                                  int mask, int link, int clip_lo, int clip_hi, int quality, int subsamp, int flags,
                                  int iters, float *ms, float *stage_ms) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = level_filter(ctx, "vf_jpeg_bench_level", rule, mask, link, clip_lo, clip_hi, &filter)) return rc;
  return jpeg_filter_bench(ctx, "vf_jpeg_bench_level", jpegs, jpeg_sizes, n, quality, subsamp, flags, iters, ms, stage_ms,
                           filter);
}

// ---- JPEG with CLAHE in place of the inversion ----------------------------------------------------------

VF_EXPORT int vf_jpeg_clahe(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n, int clip_q8,
                            int tiles_x, int tiles_y, int mask, int quality, int subsamp, int flags, uint8_t *const *outs,
                            const size_t *caps, size_t *sizes) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = clahe_filter(ctx, "vf_jpeg_clahe", clip_q8, tiles_x, tiles_y, mask, &filter)) return rc;
  return jpeg_filter(ctx, "vf_jpeg_clahe", jpegs, jpeg_sizes, n, quality, subsamp, flags, outs, caps, sizes, filter);
}

VF_EXPORT int vf_jpeg_clahe_submit(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n, int clip_q8,
                                   int tiles_x, int tiles_y, int mask, int quality, int subsamp, int flags,
                                   uint64_t *ticket) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = clahe_filter(ctx, "vf_jpeg_clahe_submit", clip_q8, tiles_x, tiles_y, mask, &filter)) return rc;
  return jpeg_filter_submit(ctx, "vf_jpeg_clahe_submit", jpegs, jpeg_sizes, n, quality, subsamp, flags, ticket, filter);
}

VF_EXPORT int vf_jpeg_bench_clahe(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n, int clip_q8,
                                  int tiles_x, int tiles_y, int mask, int quality, int subsamp, int flags, int iters,
                                  float *ms, float *stage_ms) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = clahe_filter(ctx, "vf_jpeg_bench_clahe", clip_q8, tiles_x, tiles_y, mask, &filter)) return rc;
  return jpeg_filter_bench(ctx, "vf_jpeg_bench_clahe", jpegs, jpeg_sizes, n, quality, subsamp, flags, iters, ms, stage_ms,
                           filter);
}

// ---- JPEG with the affine warp in place of the inversion ---------------------------------------------

VF_EXPORT int vf_jpeg_warp(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n, const double *m,
                           int mode, int interp, int border, const int *value, int quality, int subsamp, int flags,
                           uint8_t *const *outs, const size_t *caps, size_t *sizes) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = warp_filter(ctx, "vf_jpeg_warp", m, mode, interp, border, value, &filter)) return rc;
  return jpeg_filter(ctx, "vf_jpeg_warp", jpegs, jpeg_sizes, n, quality, subsamp, flags, outs, caps, sizes, filter);
}

VF_EXPORT int vf_jpeg_warp_submit(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n, const double *m,
                                  int mode, int interp, int border, const int *value, int quality, int subsamp, int flags,
                                  uint64_t *ticket) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = warp_filter(ctx, "vf_jpeg_warp_submit", m, mode, interp, border, value, &filter)) return rc;
  return jpeg_filter_submit(ctx, "vf_jpeg_warp_submit", jpegs, jpeg_sizes, n, quality, subsamp, flags, ticket, filter);
}

VF_EXPORT int vf_jpeg_bench_warp(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n, const double *m,
                                 int mode, int interp, int border, const int *value, int quality, int subsamp, int flags,
                                 int iters, float *ms, float *stage_ms) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = warp_filter(ctx, "vf_jpeg_bench_warp", m, mode, interp, border, value, &filter)) return rc;
  return jpeg_filter_bench(ctx, "vf_jpeg_bench_warp", jpegs, jpeg_sizes, n, quality, subsamp, flags, iters, ms, stage_ms,
                           filter);
}

// ---- JPEG with the resize in place of the inversion: the result is encoded at its own size ------------

VF_EXPORT int vf_jpeg_resize(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n, int dw, int dh,
                             double fx, double fy, int interp, int quality, int subsamp, int flags, uint8_t *const *outs,
                             const size_t *caps, size_t *sizes) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = resize_filter(ctx, "vf_jpeg_resize", dw, dh, fx, fy, interp, &filter)) return rc;
  return jpeg_filter(ctx, "vf_jpeg_resize", jpegs, jpeg_sizes, n, quality, subsamp, flags, outs, caps, sizes, filter);
}

VF_EXPORT int vf_jpeg_resize_submit(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n, int dw, int dh,
                                    double fx, double fy, int interp, int quality, int subsamp, int flags, uint64_t *ticket) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = resize_filter(ctx, "vf_jpeg_resize_submit", dw, dh, fx, fy, interp, &filter)) return rc;
  return jpeg_filter_submit(ctx, "vf_jpeg_resize_submit", jpegs, jpeg_sizes, n, quality, subsamp, flags, ticket, filter);
}

VF_EXPORT int vf_jpeg_bench_resize(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n, int dw, int dh,
                                   double fx, double fy, int interp, int quality, int subsamp, int flags, int iters, float *ms,
                                   float *stage_ms) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = resize_filter(ctx, "vf_jpeg_bench_resize", dw, dh, fx, fy, interp, &filter)) return rc;
  return jpeg_filter_bench(ctx, "vf_jpeg_bench_resize", jpegs, jpeg_sizes, n, quality, subsamp, flags, iters, ms, stage_ms,
                           filter);
}

// ---- JPEG with a filter chain in place of the inversion ---------------------------------------------

VF_EXPORT int vf_jpeg_chain(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                            const vf_step *steps, int nsteps, int quality, int subsamp, int flags, uint8_t *const *outs,
                            const size_t *caps, size_t *sizes) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = chain_filter(ctx, "vf_jpeg_chain", steps, nsteps, &filter)) return rc;
  return jpeg_filter(ctx, "vf_jpeg_chain", jpegs, jpeg_sizes, n, quality, subsamp, flags, outs, caps, sizes, filter);
}

VF_EXPORT int vf_jpeg_chain_submit(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                                   const vf_step *steps, int nsteps, int quality, int subsamp, int flags,
                                   uint64_t *ticket) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = chain_filter(ctx, "vf_jpeg_chain_submit", steps, nsteps, &filter)) return rc;
  return jpeg_filter_submit(ctx, "vf_jpeg_chain_submit", jpegs, jpeg_sizes, n, quality, subsamp, flags, ticket, filter);
}

VF_EXPORT int vf_jpeg_bench_chain(vf_ctx *ctx, const uint8_t *const *jpegs, const size_t *jpeg_sizes, int n,
                                  const vf_step *steps, int nsteps, int quality, int subsamp, int flags, int iters,
                                  float *ms, float *stage_ms) {
  VF_CHECK_CTX(ctx);
  Filter filter;
  if (const int rc = chain_filter(ctx, "vf_jpeg_bench_chain", steps, nsteps, &filter)) return rc;
  return jpeg_filter_bench(ctx, "vf_jpeg_bench_chain", jpegs, jpeg_sizes, n, quality, subsamp, flags, iters, ms,
                           stage_ms, filter);
}
