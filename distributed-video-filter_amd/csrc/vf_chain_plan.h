// vf_chain_plan.h — the plan of a filter chain (host only, no HIP, so
// tests/chain/chain_plan_check.cc checks it on the CPU).  Not installed.
//
// A program is a straight-line list of 1 .. kMaxSteps steps over values: value 0 is the input
// frame, value i the result of step i (1-based), the program's result the last step's value.  A
// step names its operand a, a binary step b as well; operands are earlier values.  From a
// validated program this file derives
//   * folding   a table step whose only reader is a table step is composed into that reader;
//   * buffers   which buffer each value lives in, assigned by last use;
//   * rows      working backwards from an output band, the rows of every value that must exist,
//               and the program's total vertical reach R;
//   * launches  per band, every step with its buffers, row offsets and row ranges: the list that
//               both GPU paths walk and the CPU check simulates;
//   * sizes     the width and height of every value: a resize step makes a value of another size
//               than its operand, every other step one of its operand's size (value_sizes); a
//               program that holds a resize step is planned on whole frames by frame_launches,
//               whose launches carry the sizes, and its buffers are as large as the largest value
//               they hold (buffer_bytes).
// Every step sees whole-frame borders: a step that makes rows [lo, hi) of its value from an
// operand of vertical radius r reads the operand's rows [lo - r, hi + r) clipped to the frame, and
// resolves its border in FRAME coordinates (vf_conv_border.h) exactly as one band of
// vf_conv_bands.h does.  So the result is what running the steps one after the other on whole
// frames gives, however the frame is cut into bands.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "vf_clahe_plan.h"
#include "vf_level_plan.h"
#include "vf_resize_plan.h"
#include "vf_warp_plan.h"

namespace vf {
namespace chain {

constexpr int kMaxSteps = 8;  // VF_CHAIN_MAX_STEPS (include/vfilter.h)
constexpr int kMaxSide = 7;   // the largest kernel or element side (conv::kMaxK)
constexpr int kMaxSepSide = 31;  // the most taps of one axis of a separable step (sep::kMaxSide)

// VF_STEP_*.  The values are not dense: 4 is left out on purpose.  Kind 4 is the value the checks
// of this file and of the C ABI have always used for "a kind that does not exist" (refused with
// "unknown kind 4"), and callers may rely on that refusal, so the colour matrix took 5.  6 and 9
// are refused in callers' checks the same way, so the separable filter took 7, the level
// filter 8 and CLAHE 10; 11 stays refused as well, so the warp took 12, and 13 stays refused, so the
// resize took 14, and 15 stays refused.
enum : int { kTable = 0, kConv = 1, kRank = 2, kBinary = 3, kMix = 5, kSep = 7, kLevel = 8, kClahe = 10, kWarp = 12, kResize = 14 };
enum : int { kRoundHalfEven = 0, kRoundHalfUp = 1 };                             // VF_ROUND_*
enum : int { kSubtract = 0, kAdd = 1, kAbsdiff = 2, kMin = 3, kMax = 4 };        // VF_BIN_*

struct Step {
  int kind = kTable;
  int a = 0, b = 0;  // operand values; b is read by a binary step only
  int op = 0;        // kRank: a VF_RANK_*; kBinary: a VF_BIN_*; kMix, kSep: a VF_ROUND_*; kLevel: a VF_LEVEL_*
  int kw = 0, kh = 0, shift = 0, border = 0;  // kConv, kRank, kSep; shift: kMix as well
  int channels = 1;                           // kTable: 1 or 3
  std::vector<uint8_t> table;    // kTable: channels x 256, planar
  std::vector<int16_t> weights;  // kConv: kw * kh
  std::vector<uint8_t> element;  // kRank: kw * kh
  std::vector<int32_t> matrix;   // kMix: 12, row-major [M | t] 3 x 4
  std::vector<int16_t> taps_x, taps_y;  // kSep: kw horizontal and kh vertical taps
  int divisor = 1;                      // kSep: odd, 1 .. 1023; 1: none
  int mask = 0, link = 0, clip_lo = 0, clip_hi = 0;  // kLevel (vf_level_plan.h); mask: kClahe as well
  int clip_q8 = 0, tiles_x = 0, tiles_y = 0;         // kClahe (vf_clahe_plan.h)
  warp::StepData warp = {};                          // kWarp (vf_warp_plan.h); border: kWarp as well
  resize::StepData resize = {};                      // kResize (vf_resize_plan.h)
};

struct Program {
  std::vector<Step> steps;  // steps[i - 1] makes value i
  int size() const { return (int)steps.size(); }
};

inline bool is_neighbourhood(const Step &s) { return s.kind == kConv || s.kind == kRank || s.kind == kSep; }
inline int radius(const Step &s) { return is_neighbourhood(s) ? s.kh / 2 : 0; }  // vertical
// A step that reads its operand at other places than the one it writes, so never in place: the
// neighbourhood steps, a warp step (radius 0: its reach is the whole frame, see whole_frame) and a
// resize step, whose result is not even of its operand's size.
inline bool reads_elsewhere(const Step &s) { return is_neighbourhood(s) || s.kind == kWarp || s.kind == kResize; }

// A level step reads its whole operand before it writes a byte (vf_level.hip), and so does a CLAHE
// step (vf_clahe.hip: every tile's table is complete before the blend starts): a program that holds
// one is planned on whole frames only, y0 = 0 and y1 = H, and never cut into bands.  A warp step
// (vf_warp.hip) reads anywhere in its operand, with the same consequence, and so does a resize step
// (vf_resize.hip), whose rows are not its operand's rows.
inline bool has_resize(const Program &p) {
  for (const Step &s : p.steps)
    if (s.kind == kResize) return true;
  return false;
}
inline bool whole_frame(const Program &p) {
  for (const Step &s : p.steps)
    if (s.kind == kLevel || s.kind == kClahe || s.kind == kWarp) return true;
  return has_resize(p);
}

// The device scratch of a whole-frame program's steps (run_launches' hist), in bytes: the level
// steps' histogram words, level::kHistWords for each step of the program (step i's at (i - 1) *
// kHistWords), then one clahe::kScratchBytes for each CLAHE step, in the steps' order.
inline size_t level_scratch_bytes() { return (size_t)kMaxSteps * level::kHistWords * sizeof(uint32_t); }
inline int clahe_steps_before(const Program &p, int step) {  // step: 1-based
  int k = 0;
  for (int i = 1; i < step && i <= p.size(); ++i) k += p.steps[i - 1].kind == kClahe;
  return k;
}
inline size_t whole_frame_scratch_bytes(const Program &p) {
  return level_scratch_bytes() + (size_t)clahe_steps_before(p, p.size() + 1) * clahe::kScratchBytes;
}

// Is value v read by step s?
inline bool reads(const Step &s, int v) { return s.a == v || (s.kind == kBinary && s.b == v); }

// The structure of a program for frames of `frame_channels` channels.  false with the reason in
// *why.  The contents of a table, a kernel or an element are the single-filter checks' business.
inline bool validate(const Program &p, int frame_channels, std::string *why) {
  const int n = p.size();
  auto fail = [&](const std::string &m) {
    if (why) *why = m;
    return false;
  };
  if (n < 1) return fail("an empty program");
  if (n > kMaxSteps)
    return fail("a program of " + std::to_string(n) + " steps; at most " + std::to_string(kMaxSteps));
  if (frame_channels != 1 && frame_channels != 3) return fail("frames have 1 or 3 channels");
  for (int i = 1; i <= n; ++i) {
    const Step &s = p.steps[i - 1];
    const std::string at = "step " + std::to_string(i) + ": ";
    if ((s.kind < kTable || s.kind > kBinary) && s.kind != kMix && s.kind != kSep && s.kind != kLevel && s.kind != kClahe &&
        s.kind != kWarp && s.kind != kResize)
      return fail(at + "unknown kind " + std::to_string(s.kind));
    if (s.a < 0 || s.a >= i)
      return fail(at + "operand a = " + std::to_string(s.a) + " is not an earlier value");
    if (s.kind == kBinary) {
      if (s.b < 0 || s.b >= i)
        return fail(at + "operand b = " + std::to_string(s.b) + " is not an earlier value");
      if (s.op < kSubtract || s.op > kMax) return fail(at + "unknown binary op " + std::to_string(s.op));
    }
    if (s.kind == kTable) {
      if (s.channels != 1 && s.channels != 3) return fail(at + "a table has 1 or 3 channels");
      if (s.table.size() != (size_t)s.channels * 256) return fail(at + "a table holds channels x 256 bytes");
      if (s.channels == 3 && frame_channels != 3) return fail(at + "a 3-channel table on 1-channel frames");
    }
    if (s.kind == kMix) {
      if (frame_channels != 3) return fail(at + "a colour matrix on 1-channel frames");
      if (s.matrix.size() != 12) return fail(at + "a colour matrix holds 3 x 4 entries");
      if (s.op != kRoundHalfEven && s.op != kRoundHalfUp) return fail(at + "unknown rounding " + std::to_string(s.op));
    }
    if (s.kind == kLevel) {
      std::string m;
      if (!level::limits_ok(s.op, s.mask, s.link, s.clip_lo, s.clip_hi, frame_channels, &m)) return fail(at + m);
    }
    if (s.kind == kClahe) {
      std::string m;
      if (!clahe::limits_ok(s.clip_q8, s.tiles_x, s.tiles_y, s.mask, frame_channels, &m)) return fail(at + m);
    }
    if (s.kind == kWarp) {
      std::string m;
      const int value[3] = {s.warp.value[0], s.warp.value[1], s.warp.value[2]};
      if (!warp::limits_ok(s.warp.m, s.warp.mode, s.warp.interp, s.border, value, frame_channels, &m)) return fail(at + m);
    }
    if (s.kind == kResize) {
      std::string m;
      if (!resize::limits_ok(s.resize.dw, s.resize.dh, s.resize.fx, s.resize.fy, s.resize.interp, frame_channels, &m))
        return fail(at + m);
    }
    if (s.kind == kSep) {
      if (s.kw < 1 || s.kh < 1 || s.kw > kMaxSepSide || s.kh > kMaxSepSide || !(s.kw & 1) || !(s.kh & 1))
        return fail(at + "a separable step's tap counts are odd and at most " + std::to_string(kMaxSepSide));
      if (s.taps_x.size() != (size_t)s.kw || s.taps_y.size() != (size_t)s.kh)
        return fail(at + "the taps do not hold kw and kh entries");
      if (s.op != kRoundHalfEven && s.op != kRoundHalfUp) return fail(at + "unknown rounding " + std::to_string(s.op));
    } else if (is_neighbourhood(s)) {
      if (s.kw < 1 || s.kh < 1 || s.kw > kMaxSide || s.kh > kMaxSide || !(s.kw & 1) || !(s.kh & 1))
        return fail(at + "sides are odd and at most " + std::to_string(kMaxSide));
      const size_t count = (size_t)s.kw * (size_t)s.kh;
      if (s.kind == kConv ? s.weights.size() != count : s.element.size() != count)
        return fail(at + "the kernel or element does not hold kw x kh entries");
    }
  }
  for (int v = 0; v < n; ++v) {  // every value but the last is read
    bool read = false;
    for (int i = v + 1; i <= n && !read; ++i) read = reads(p.steps[i - 1], v);
    if (!read) return fail("value " + std::to_string(v) + " is read by no step (a dead value)");
  }
  return true;
}

// ---- folding -------------------------------------------------------------------------------------

// then(first(v)) per channel: channels = 3 when either has 3.
inline void compose_tables(const Step &first, const Step &then, Step *out) {
  const int ch = first.channels == 3 || then.channels == 3 ? 3 : 1;
  std::vector<uint8_t> t((size_t)ch * 256);
  for (int c = 0; c < ch; ++c) {
    const uint8_t *f = first.table.data() + (first.channels == 3 ? 256 * c : 0);
    const uint8_t *g = then.table.data() + (then.channels == 3 ? 256 * c : 0);
    for (int v = 0; v < 256; ++v) t[(size_t)c * 256 + v] = g[f[v]];
  }
  out->channels = ch;
  out->table = std::move(t);
}

// The program with every table step whose only reader is a table step composed into that reader
// (exact: both are per-byte maps).  The result computes the same picture in fewer steps.  Nothing
// is composed across a colour matrix: a table beside one stays a step, and two matrices with a
// rounding and a clamp between them are not one matrix.  Nor across a separable, a level or a CLAHE
// step: only table steps are ever composed, and a level or CLAHE step's tables do not exist before
// the frame does.  Nor across a warp step: a table before one is not a table after one when the
// constant border's colour enters the blend.  Nor across a resize step: only neighbouring table steps
// are ever composed, and a table step on each side of one reads and is read by the resize step.
inline Program fold(const Program &in) {
  Program p = in;
  for (bool again = true; again;) {
    again = false;
    const int n = p.size();
    for (int i = 1; i < n && !again; ++i) {
      if (p.steps[i - 1].kind != kTable) continue;
      int readers = 0, reader = 0;
      for (int j = i + 1; j <= n; ++j)
        if (reads(p.steps[j - 1], i)) ++readers, reader = j;
      if (readers != 1 || p.steps[reader - 1].kind != kTable) continue;
      Step &r = p.steps[reader - 1];
      compose_tables(p.steps[i - 1], r, &r);
      r.a = p.steps[i - 1].a;
      p.steps.erase(p.steps.begin() + (i - 1));
      for (Step &s : p.steps) {  // values above i move down by one
        if (s.a > i) --s.a;
        if (s.b > i) --s.b;
      }
      again = true;
    }
  }
  return p;
}

// The kind a (folded) program may run as when it is one step on value 0 that is not binary, else
// -1: a program that folds to one table step takes the JPEG path's fused colour stage.
inline int single_kind(const Program &p) {
  if (p.size() != 1 || p.steps[0].kind == kBinary || p.steps[0].a != 0) return -1;
  return p.steps[0].kind;
}

// ---- buffers -------------------------------------------------------------------------------------

struct Buffers {
  std::vector<int> of;  // of[v]: the buffer of value v; of[0] == 0
  int count = 0;        // buffers used
  int result = 0;       // the buffer of the program's result
};

// Buffers by last use.  Buffer 0 holds value 0 and is reused once value 0 is dead.  A
// neighbourhood step never writes the buffer it reads; a table, colour-matrix or binary step writes
// in place over an operand that dies at that step (a separable step is a neighbourhood step: never
// in place; a level or CLAHE step is not one: its histograms are complete before its first byte is
// written; a warp step reads anywhere in its operand: never in place either, reads_elsewhere).  Every
// value of a buffer sits at one row origin (the band's
// first source row), so "in place" is dst == operand exactly.
// keep_input: buffer 0 holds value 0 and nothing else, ever (the JPEG path under a resize step: the
// decoded frames lie in buffer 0 at the decoder's offsets, one frame's bytes each, and a later value
// may be larger than its frame).
inline Buffers assign_buffers(const Program &p, bool keep_input = false) {
  const int n = p.size();
  std::vector<int> last(n + 1, 0);  // the last step that reads value v; the result outlives all
  for (int i = 1; i <= n; ++i) {
    last[p.steps[i - 1].a] = i;
    if (p.steps[i - 1].kind == kBinary) last[p.steps[i - 1].b] = i;
  }
  last[n] = n + 1;
  Buffers out;
  out.of.assign(n + 1, 0);
  std::vector<int> holder_dies{keep_input ? n + 1 : last[0]};  // per buffer: the last read of the value it holds
  for (int i = 1; i <= n; ++i) {
    const Step &s = p.steps[i - 1];
    int pick = -1;
    if (!reads_elsewhere(s)) {  // in place over an operand that dies here
      if (last[s.a] == i) pick = out.of[s.a];
      else if (s.kind == kBinary && last[s.b] == i) pick = out.of[s.b];
      if (keep_input && pick == 0) pick = -1;
    }
    for (int k = 0; pick < 0 && k < (int)holder_dies.size(); ++k)
      if (holder_dies[k] < i) pick = k;  // its value is dead: no step from i on reads it
    if (pick < 0) {
      pick = (int)holder_dies.size();
      holder_dies.push_back(0);
    }
    out.of[i] = pick;
    holder_dies[pick] = keep_input && pick == 0 ? n + 1 : last[i];
  }
  out.count = (int)holder_dies.size();
  out.result = out.of[n];
  return out;
}

// ---- reach and row ranges ------------------------------------------------------------------------

struct Rows {
  int lo = 0, hi = 0;  // rows [lo, hi)
};

// The rows of every value that must exist for rows [y0, y1) of the result of a frame of H rows
// (0 <= y0 < y1 <= H): out[v] for v = 0 .. n.  out[0] is the upload.  A level, CLAHE or warp step has whole-frame
// reach, so a program that holds one asks for all H rows of every value, whatever [y0, y1) is.
inline std::vector<Rows> rows_needed(const Program &p, int H, int y0, int y1) {
  const int n = p.size();
  std::vector<Rows> need(n + 1);
  if (whole_frame(p)) {
    for (Rows &r : need) r.lo = 0, r.hi = H;
    return need;
  }
  std::vector<bool> have(n + 1, false);
  need[n].lo = y0;
  need[n].hi = y1;
  have[n] = true;
  auto want = [&](int v, int lo, int hi) {
    if (lo < 0) lo = 0;
    if (hi > H) hi = H;
    if (!have[v]) {
      need[v].lo = lo;
      need[v].hi = hi;
      have[v] = true;
    } else {  // every range holds [y0, y1), so a union of ranges is a range
      if (lo < need[v].lo) need[v].lo = lo;
      if (hi > need[v].hi) need[v].hi = hi;
    }
  };
  for (int i = n; i >= 1; --i) {
    const Step &s = p.steps[i - 1];
    if (!have[i]) continue;  // a dead value: validate() refuses those
    const int r = radius(s);
    want(s.a, need[i].lo - r, need[i].hi + r);
    if (s.kind == kBinary) want(s.b, need[i].lo - r, need[i].hi + r);
  }
  return need;
}

// The program's total vertical reach: the largest summed radius along a path from the result to
// value 0.  Rows [y0, y1) of the result read rows [y0 - R, y1 + R) of the input at the most.
inline int reach(const Program &p) {
  const int n = p.size();
  std::vector<int> r(n + 1, -1);
  r[n] = 0;
  for (int i = n; i >= 1; --i) {
    if (r[i] < 0) continue;
    const Step &s = p.steps[i - 1];
    const int t = r[i] + radius(s);
    if (t > r[s.a]) r[s.a] = t;
    if (s.kind == kBinary && t > r[s.b]) r[s.b] = t;
  }
  return r[0] < 0 ? 0 : r[0];
}

// ---- launches ------------------------------------------------------------------------------------

constexpr int kOut = -1;  // Launch::dst_buf: the caller's output rows, not a buffer

// One step of one band, fully addressed for its kernel (run_launches, vf_api.hip).  Every
// buffer holds its value's row y at row y - s0, s0 the band's origin row.
struct Launch {
  int step;                   // 1-based; prog.steps[step - 1]
  int a_buf, b_buf;           // buffers of the operands (b_buf read by binary steps only)
  int dst_buf;                // buffer of the result, or kOut
  int a_row, b_row, dst_row;  // first row handed to the kernel, relative to s0
  int y0, nrows;              // the rows of this value to make (frame coordinates)
  int src0, nsrc;             // the operand's first row handed over and the count (launch_conv's s0, nsrc)
  int a_w = 0, a_h = 0;       // frame_launches only: the operand's size (a binary step's two operands agree) ...
  int w = 0, h = 0;           // ... and the result's; 0 from band_launches: every value has the frame's size
};

// The launches that make rows [y0, y1) of the result for a frame of H rows whose buffers start at
// row s0 (the whole frame: y0 = 0, y1 = H, s0 = 0).  A table, colour-matrix or binary step
// reads its operands at its own first row; a neighbourhood step gets every present row of its
// operand.  With result_to_out the last step writes row 0 of the caller's output, else its
// planned buffer.
inline std::vector<Launch> band_launches(const Program &p, const Buffers &bufs, int H, int y0, int y1, int s0,
                                         bool result_to_out) {
  const int n = p.size();
  const std::vector<Rows> need = rows_needed(p, H, y0, y1);
  std::vector<Launch> out;
  for (int i = 1; i <= n; ++i) {
    const Step &s = p.steps[i - 1];
    const Rows r = need[i], src = is_neighbourhood(s) ? need[s.a] : r;
    const bool to_out = result_to_out && i == n;
    out.push_back(Launch{i, bufs.of[s.a], bufs.of[s.kind == kBinary ? s.b : s.a], to_out ? kOut : bufs.of[i], src.lo - s0,
                         r.lo - s0, to_out ? 0 : r.lo - s0, r.lo, r.hi - r.lo, src.lo, src.hi - src.lo});
  }
  return out;
}

// ---- sizes ---------------------------------------------------------------------------------------

struct Size {
  int w = 0, h = 0;
};

// The size of every value for a frame of W x H (each at least 1): out[v] for v = 0 .. n.  A resize
// step makes resize::out_size of its operand's size; every other step a value of its operand's size.
// false with the reason in *why, naming the step: a resize step that refuses its operand's size
// (resize::frame_ok), or a binary step whose operands differ in size.
inline bool value_sizes(const Program &p, int W, int H, std::vector<Size> *out, std::string *why) {
  const int n = p.size();
  out->assign((size_t)n + 1, Size{});
  (*out)[0].w = W, (*out)[0].h = H;
  for (int i = 1; i <= n; ++i) {
    const Step &s = p.steps[i - 1];
    const Size a = (*out)[s.a];
    const std::string at = "step " + std::to_string(i) + ": ";
    Size r = a;
    if (s.kind == kResize) {
      std::string m;
      resize::Plan plan;
      if (!resize::frame_ok((uint64_t)a.w, (uint64_t)a.h, s.resize.dw, s.resize.dh, s.resize.fx, s.resize.fy, s.resize.interp,
                            &plan, &m)) {
        if (why) *why = at + m;
        return false;
      }
      r.w = plan.dw, r.h = plan.dh;
    } else if (s.kind == kBinary) {
      const Size b = (*out)[s.b];
      if (a.w != b.w || a.h != b.h) {
        if (why)
          *why = at + "operand a (value " + std::to_string(s.a) + ") is " + std::to_string(a.w) + " x " + std::to_string(a.h) +
                 " and operand b (value " + std::to_string(s.b) + ") is " + std::to_string(b.w) + " x " + std::to_string(b.h) +
                 ": a binary step's operands have one size";
        return false;
      }
    }
    (*out)[i] = r;
  }
  return true;
}

// The whole-frame launches of a program whose values have `sizes` (value_sizes): band_launches'
// list for y0 = 0, y1 = H and s0 = 0, with every row count taken from the value it belongs to and
// each launch carrying its operand's and its result's size.  For a program without a resize step
// the first eleven members equal band_launches(p, bufs, H, 0, H, 0, result_to_out)'s.
inline std::vector<Launch> frame_launches(const Program &p, const Buffers &bufs, const std::vector<Size> &sizes,
                                          bool result_to_out) {
  const int n = p.size();
  std::vector<Launch> out;
  for (int i = 1; i <= n; ++i) {
    const Step &s = p.steps[i - 1];
    const bool to_out = result_to_out && i == n;
    const Size a = sizes[s.a], r = sizes[i];
    out.push_back(Launch{i, bufs.of[s.a], bufs.of[s.kind == kBinary ? s.b : s.a], to_out ? kOut : bufs.of[i], 0, 0, 0, 0, r.h, 0,
                         is_neighbourhood(s) ? a.h : r.h, a.w, a.h, r.w, r.h});
  }
  return out;
}

// The bytes of each buffer: those of the largest value it holds, at `channels` bytes a pixel.
inline std::vector<size_t> buffer_bytes(const Buffers &bufs, const std::vector<Size> &sizes, int channels) {
  std::vector<size_t> out((size_t)bufs.count, 0);
  for (size_t v = 0; v < sizes.size() && v < bufs.of.size(); ++v) {
    const size_t bytes = (size_t)sizes[v].w * (size_t)sizes[v].h * (size_t)channels;
    out[(size_t)bufs.of[v]] = std::max(out[(size_t)bufs.of[v]], bytes);
  }
  return out;
}

// The buffers beyond buffer 0 that some launch addresses: bufs.count - 1 when the result stays in
// its buffer, 0 for a one-step program whose result goes to the caller's output.
inline int scratch_buffers(const Buffers &bufs, const Program &p, bool result_to_out) {
  int top = 0;
  for (const Launch &l : band_launches(p, bufs, 1, 0, 1, 0, result_to_out))
    top = std::max({top, l.a_buf, l.b_buf, l.dst_buf});
  return top;
}

}  // namespace chain
}  // namespace vf
