// vf_jpeg_plan.h — which variant of each decode stage a JPEG batch runs.  The codec reads the
// VF_JPEG_* switches once at the top of an entry call (JpegSwitches::read), learns the batch's
// traits in prepare_decode and resolves both into one DecodePlan; everything that runs later,
// the resync after a wait on another thread included, reads the plan and never the environment.
// Host-only, no HIP: tests/plan/jpeg_plan_check.cc exercises resolve() under g++.
// Not installed.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "vf_env.h"
#include "vf_jpeg_types.h"

namespace vf {
namespace jpeg {

// The raw values of the codec's per-call switches (nullptr: unset); INTEGRATION.md lists them.
// The pointers are the environment's own, good until it changes: a JpegSwitches lives for its
// entry call only, and resolve() keeps none of them.
struct JpegSwitches {
  const char *sync = nullptr;         // VF_JPEG_SYNC
  const char *sync_lsb = nullptr;     // VF_JPEG_SYNC_LSB
  const char *sync_tabs4 = nullptr;   // VF_JPEG_SYNC_TABS4
  const char *sync_g = nullptr;       // VF_JPEG_SYNC_G
  const char *sync_queued = nullptr;  // VF_JPEG_SYNC_QUEUED
  const char *sync_warm = nullptr;    // VF_JPEG_SYNC_WARM
  const char *sync_stats = nullptr;   // VF_JPEG_SYNC_STATS
  const char *chunks = nullptr;       // VF_JPEG_CHUNKS
  const char *write4 = nullptr;       // VF_JPEG_WRITE4
  const char *fuse = nullptr;         // VF_JPEG_FUSE
  const char *fuse_idct = nullptr;    // VF_JPEG_FUSE_IDCT
  const char *idct24 = nullptr;       // VF_JPEG_IDCT24
  const char *fetch_learn = nullptr;  // VF_JPEG_FETCH_LEARN
  const char *trace = nullptr;        // VF_JPEG_TRACE

  // the only code that reads these names; per entry call: tests and A/Bs switch them inside one process
  static JpegSwitches read() {
    JpegSwitches s;
    s.sync = env_str("VF_JPEG_SYNC");
    s.sync_lsb = env_str("VF_JPEG_SYNC_LSB");
    s.sync_tabs4 = env_str("VF_JPEG_SYNC_TABS4");
    s.sync_g = env_str("VF_JPEG_SYNC_G");
    s.sync_queued = env_str("VF_JPEG_SYNC_QUEUED");
    s.sync_warm = env_str("VF_JPEG_SYNC_WARM");
    s.sync_stats = env_str("VF_JPEG_SYNC_STATS");
    s.chunks = env_str("VF_JPEG_CHUNKS");
    s.write4 = env_str("VF_JPEG_WRITE4");
    s.fuse = env_str("VF_JPEG_FUSE");
    s.fuse_idct = env_str("VF_JPEG_FUSE_IDCT");
    s.idct24 = env_str("VF_JPEG_IDCT24");
    s.fetch_learn = env_str("VF_JPEG_FETCH_LEARN");
    s.trace = env_str("VF_JPEG_TRACE");
    return s;
  }
};

// What prepare_decode learns about the batch and the selection depends on.
struct BatchTraits {
  bool spec_ok = true;   // every frame fits the speculative resolver
  bool tabs4 = true;     // every frame fits the span sync's 4-table layout (DecFrame::tabs4)
  bool pow2bpm = true;   // every frame's blocks per MCU divide 16 (the syncs' LSB-first lanes)
  bool d422 = true;      // every frame is standard 4:2:2 (k_idct_color422)
  uint32_t max_sub = 0;  // subsequences of the largest entropy-coded segment
  uint64_t bits_per_block = 0;  // the batch's entropy-coded bits per block
};

struct DecodePlan {
  bool spec = false;    // the speculative sync; else the pass-based one:
  int g = 4;            //   spans of g subsequences per thread (k_syncg), 0: the host-looped k_sync
  int tabs = 0;         //   k_syncg's table layout: 0 six tables, 1 four, 2 four with the LSB-first lane
  int queued = kQueuedPasses;  // span passes queued before the host checks convergence
  uint32_t warm = 0;    //   bits a span-sync thread decodes before its span in pass 0
  bool lsb = false;     // the LSB-first lanes (both syncs)
  bool chunks = false;  // write pass: 16-B coefficient rows + row masks; else a cleared buffer
  bool write4 = true;   // four lanes per subsequence in the write pass after span passes
  bool fuse = false;    // invert path: the colour pass writes the encoder's sample planes
  bool fuse_idct = false;  // ... and IDCT + colour run as one pass (k_idct_color422)
  bool enc_fast = false;   // invert path: the encoder's DCT (kFlagFastDct), set by the codec
  bool stats = false;   // VF_JPEG_SYNC_STATS counters on stderr
  bool trace = false;   // VF_JPEG_TRACE host phases on stderr
};

// The batch's plan from the switches and its traits: a pure function (no environment, no codec
// state).  fuse_requested: the call is an invert, whose decoder may feed the encoder directly.
inline DecodePlan resolve(const JpegSwitches &sw, const BatchTraits &t, bool fuse_requested) {
  DecodePlan p;
  // VF_JPEG_SYNC = spec | pass | auto (default).  auto: speculative for frames of up to
  // kSpecAutoSubs subsequences (measured, MI355X, q85 4:2:2 batches of 32: 480p 50.4k vs 37.6k
  // fps, 1080p 18.0k vs 17.2k; 4K 5.48k vs 5.65k, where the bpm-fold trajectory decode costs
  // more than the pass chains it removes).  A batch the resolver cannot stage (spec_ok) takes
  // the passes whatever the switch says.
  constexpr uint32_t kSpecAutoSubs = 12288;
  const bool force_pass = sw.sync && std::strcmp(sw.sync, "pass") == 0;
  const bool force_spec = sw.sync && std::strcmp(sw.sync, "spec") == 0;
  p.spec = t.spec_ok && !force_pass && (force_spec || t.max_sub <= kSpecAutoSubs);
  // the LSB-first lanes (SpanLaneRT) when every frame's block cycle divides 16 (k_spec's
  // 2-bit component slots; k_syncg's 1-bit table slots need it to divide 32); VF_JPEG_SYNC_LSB=0: off
  p.lsb = t.pow2bpm && flag_on(sw.sync_lsb);
  // pass-based: spans of G subsequences per thread (VF_JPEG_SYNC_G = 1, 2, 3, 4, 8; 0 = the
  // host-looped one-subsequence k_sync).  With every frame on 4 table slots (DecFrame::tabs4;
  // VF_JPEG_SYNC_TABS4=0 turns it off) the span sync's LDS leaves room for G = 5 at 3 workgroups
  // per CU: 25 % more stream resident.  dec_syncg instantiates (g, tabs) = (1 2 3 4 8, 0),
  // (4 5, 1), (4 5, 2) and nothing else: 5 without the four tables, and any other number, run as 4.
  const bool t4 = t.tabs4 && flag_on(sw.sync_tabs4);
  const int g = sw.sync_g ? std::atoi(sw.sync_g) : 5;
  p.g = g == 5 ? (t4 ? 5 : 4) : (g >= 0 && g <= 4) || g == 8 ? g : 4;
  p.tabs = t4 && (p.g == 4 || p.g == 5) ? (p.lsb ? 2 : 1) : 0;
  // VF_JPEG_SYNC_QUEUED = 1..kQueuedPasses (tests): fewer queued passes, so check_decode
  // reports them unconverged and finish_sync runs the rest
  p.queued = sw.sync_queued ? std::min(std::max(std::atoi(sw.sync_queued), 1), kQueuedPasses) : kQueuedPasses;
  // Bits a span-sync thread decodes before its span in pass 0, so that its entry is (usually)
  // synchronised already: 12 blocks' worth of the batch's bits per block -- the full state (bit
  // position, zigzag index, block-in-MCU) resynchronises at block boundaries (hard 1080p: ~250
  // bits per block, 3,008 bits of warm-up; 4K scenes: ~20, 240).  12 rather than 8 blocks: hard
  // 1080p sync 4-9 % shorter on each of four content seeds, 4K scenes unchanged
  // (profiles/r05_jpeg_sync_warm_ab.txt).  VF_JPEG_SYNC_WARM=<bits> overrides (0: guessed
  // entries); the launcher clamps it to what a workgroup stages.
  if (sw.sync_warm && *sw.sync_warm && std::strcmp(sw.sync_warm, "auto") != 0)
    p.warm = (uint32_t)std::strtoul(sw.sync_warm, nullptr, 10);
  else
    p.warm = (uint32_t)std::min<uint64_t>(4096, 12 * t.bits_per_block) & ~31u;
  // The write pass stores whole 16-B coefficient rows with a per-block mask of the rows stored,
  // which the IDCT reads: no clear of the coefficient buffer (134 MB per 1080p batch, 1.06 GB
  // per 4K one).  After the speculative sync always (k_write + clear 118 -> 105 us at 1080p).
  // After the pass-based sync only when blocks are short: its write pass runs 4 lanes per
  // subsequence, each of which decodes on to its last block's end and skips its first, which
  // costs a block per lane -- on hard content (~500 bits per block) k_write4 342 -> 1227 us,
  // on 4K scenes (~22 bits per block) huffman_write 0.50 -> 0.29 ms, resident 11.1 -> 12.0 k fps
  // (profiles/r04_jpeg_fuse_chunks_warm_ab.txt, r04_jpeg_chunks_4k_ab.txt).  VF_JPEG_CHUNKS=0 / 1
  // forces either form.
  constexpr uint64_t kChunkBitsPerBlock = 128;
  p.chunks = sw.chunks && *sw.chunks ? std::strcmp(sw.chunks, "0") != 0
                                     : p.spec || t.bits_per_block <= kChunkBitsPerBlock;
  // after the pass-based sync, every subsequence's checkpoints are states of the true path: the
  // write pass runs 4 lanes per subsequence from them (VF_JPEG_WRITE4=0: one lane)
  p.write4 = flag_on(sw.write4);
  // The invert path's fused colour pass (k_color writes the encoder's sample planes, k_fdct reads
  // them); VF_JPEG_FUSE=0 keeps the pixel round trip.  On standard 4:2:2 frames IDCT and colour
  // then run as one pass with the decoder planes in LDS (VF_JPEG_FUSE_IDCT=0: two passes).
  p.fuse = fuse_requested && flag_on(sw.fuse);
  p.fuse_idct = p.fuse && t.d422 && flag_on(sw.fuse_idct);
  p.stats = sw.sync_stats != nullptr;
  p.trace = sw.trace != nullptr;
  return p;
}

}  // namespace jpeg
}  // namespace vf
