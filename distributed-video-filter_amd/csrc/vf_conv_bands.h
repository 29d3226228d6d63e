// vf_conv_bands.h — how vf_conv_frames_host cuts a frame that does not fit its staging buffers
// into bands of rows (host only, no HIP, so tests/conv/conv_bands_check.cc checks it on the CPU).
// Not installed.
//
// A band is a run of output rows [y0, y1).  Its taps reach ry rows above and below, so the source
// rows uploaded for it are [max(0, y0 - ry), min(H, y1 + ry)): every row a tap of the band can
// resolve to under any of the three borders (a reflection of a row above the frame lands within
// ry rows of the top, and a frame shorter than ry is uploaded whole).  The border is resolved in
// FRAME coordinates (vf_conv_border.h) and only then moved into the band by subtracting s0: a band
// that starts at row 5 does not reflect at its own top.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace vf {
namespace conv {

struct Band {
  int y0, y1;  // output rows [y0, y1)
  int s0, s1;  // source rows uploaded [s0, s1); s0 is the frame row of the first one
};

// The bands of a W x H x C frame (packed rows of W * C bytes) for a kernel of vertical radius ry
// whose source rows must fit `capacity` bytes: they tile [0, H) once and in order, each as tall
// as fits.  false (and no bands) when the arguments are invalid or when some output row with its
// halo does not fit the capacity.
inline bool bands(int W, int H, int C, int ry, size_t capacity, std::vector<Band> *out) {
  out->clear();
  if (W <= 0 || H <= 0 || C <= 0 || ry < 0) return false;
  const size_t row = (size_t)W * (size_t)C;
  const size_t fit = capacity / row;  // whole source rows that fit
  const long rows = fit > (size_t)H ? (long)H : (long)fit;
  for (long y0 = 0; y0 < H;) {
    const long s0 = y0 > ry ? y0 - ry : 0;
    long y1;
    if (s0 + rows >= H) {
      y1 = H;  // the rest of the frame fits
    } else {
      y1 = s0 + rows - ry;  // y1 + ry == s0 + rows < H
    }
    if (y1 <= y0) return out->clear(), false;  // not one output row with its halo
    const long s1 = y1 + ry < H ? y1 + ry : H;
    out->push_back(Band{(int)y0, (int)y1, (int)s0, (int)s1});
    y0 = y1;
  }
  return true;
}

}  // namespace conv
}  // namespace vf
