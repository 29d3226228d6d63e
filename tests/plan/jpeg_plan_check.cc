// Checks of the JPEG decode plan (csrc/vf_jpeg_plan.h) -- test infrastructure, built by
// tests/test_jpeg_plan.py with g++ (-fsanitize=address,undefined), never part of the library.
//   jpeg_plan_check rules        every selection rule of resolve(), case by case
//   jpeg_plan_check exhaustive   every (G, TABS4, LSB, tabs4, pow2bpm): a form dec_syncg instantiates
//   jpeg_plan_check read         JpegSwitches::read() of this process's environment, one line per switch
// The first two fill JpegSwitches directly: resolve() takes no environment.
#include <cstdio>
#include <cstring>
#include <string>

#include "vf_jpeg_plan.h"

using vf::jpeg::BatchTraits;
using vf::jpeg::DecodePlan;
using vf::jpeg::JpegSwitches;
using vf::jpeg::kQueuedPasses;
using vf::jpeg::resolve;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    ++g_checks;                                                         \
    if (!(cond)) {                                                      \
      ++g_failed;                                                       \
      std::fprintf(stderr, "line %d: CHECK(%s) failed\n", __LINE__, #cond); \
    }                                                                   \
  } while (0)

// traits of a batch on which every variant is available
static BatchTraits easy() {
  BatchTraits t;
  t.max_sub = 1000;
  t.bits_per_block = 40;
  return t;
}

static int rules() {
  const JpegSwitches none;
  {  // defaults: nothing set, an easy batch, the invert path
    const DecodePlan p = resolve(none, easy(), true);
    CHECK(p.spec && p.lsb && p.g == 5 && p.tabs == 2 && p.queued == kQueuedPasses);
    CHECK(p.warm == 480 && p.chunks && p.write4 && p.fuse && p.fuse_idct && !p.enc_fast && !p.stats && !p.trace);
    const DecodePlan d = resolve(none, easy(), false);  // a plain decode never feeds the encoder
    CHECK(!d.fuse && !d.fuse_idct);
  }
  {  // sync path
    JpegSwitches s;
    BatchTraits t = easy();
    t.max_sub = 12288;
    CHECK(resolve(s, t, true).spec);  // auto: up to 12,288 subsequences
    t.max_sub = 12289;
    CHECK(!resolve(s, t, true).spec);
    s.sync = "spec";
    CHECK(resolve(s, t, true).spec);  // forced past the auto threshold
    t.spec_ok = false;
    CHECK(!resolve(s, t, true).spec);  // spec with spec_ok = false takes the span path
    t = easy();
    t.spec_ok = false;
    CHECK(!resolve(none, t, true).spec);
    s.sync = "pass";
    CHECK(!resolve(s, easy(), true).spec);
    s.sync = "auto";
    CHECK(resolve(s, easy(), true).spec);
    s.sync = "";
    CHECK(resolve(s, easy(), true).spec);
  }
  {  // lsb = pow2bpm && switch != "0"; t4 = tabs4 && switch != "0" (seen through G and the layout)
    JpegSwitches s;
    BatchTraits t = easy();
    CHECK(resolve(s, t, true).lsb);
    s.sync_lsb = "1";
    CHECK(resolve(s, t, true).lsb);
    s.sync_lsb = "0";
    CHECK(!resolve(s, t, true).lsb && resolve(s, t, true).tabs == 1);
    s.sync_lsb = nullptr;
    t.pow2bpm = false;
    CHECK(!resolve(s, t, true).lsb && resolve(s, t, true).tabs == 1);
    s.sync_tabs4 = "0";
    CHECK(resolve(s, easy(), true).g == 4 && resolve(s, easy(), true).tabs == 0);
    s.sync_tabs4 = "1";
    CHECK(resolve(s, easy(), true).g == 5 && resolve(s, easy(), true).tabs == 2);
    t = easy();
    t.tabs4 = false;
    CHECK(resolve(s, t, true).g == 4 && resolve(s, t, true).tabs == 0);
  }
  {  // G and the table layout
    struct { const char *v; bool tabs4; int g, tabs; } cases[] = {
        {nullptr, true, 5, 2}, {nullptr, false, 4, 0}, {"5", true, 5, 2}, {"5", false, 4, 0},
        {"0", true, 0, 0},     {"1", true, 1, 0},      {"2", true, 2, 0}, {"3", true, 3, 0},
        {"4", true, 4, 2},     {"4", false, 4, 0},     {"8", true, 8, 0}, {"8", false, 8, 0},
        {"6", true, 4, 2},     {"7", true, 4, 2},      {"7", false, 4, 0}, {"9", true, 4, 2},
        {"-1", true, 4, 2},    {"-1", false, 4, 0},    {"64", true, 4, 2}};
    for (const auto &c : cases) {
      JpegSwitches s;
      s.sync_g = c.v;
      BatchTraits t = easy();
      t.tabs4 = c.tabs4;
      const DecodePlan p = resolve(s, t, true);
      CHECK(p.g == c.g && p.tabs == c.tabs);
      s.sync_lsb = "0";  // the MSB lanes: layout 1 wherever it was 2
      CHECK(resolve(s, t, true).g == c.g && resolve(s, t, true).tabs == (c.tabs == 2 ? 1 : c.tabs));
    }
  }
  {  // queued passes: clamped to [1, kQueuedPasses]
    JpegSwitches s;
    CHECK(resolve(s, easy(), true).queued == kQueuedPasses);
    s.sync_queued = "0";
    CHECK(resolve(s, easy(), true).queued == 1);
    s.sync_queued = "-3";
    CHECK(resolve(s, easy(), true).queued == 1);
    s.sync_queued = "2";
    CHECK(resolve(s, easy(), true).queued == 2);
    s.sync_queued = "99";
    CHECK(resolve(s, easy(), true).queued == kQueuedPasses);
  }
  {  // warm-up bits: unset, "" and "auto" give min(4096, 12 * bits_per_block) & ~31
    JpegSwitches s;
    BatchTraits t = easy();
    for (const char *v : {(const char *)nullptr, "", "auto"}) {
      s.sync_warm = v;
      t.bits_per_block = 40;
      CHECK(resolve(s, t, true).warm == 480);
      t.bits_per_block = 251;  // 3,012 bits, rounded down to whole words
      CHECK(resolve(s, t, true).warm == 3008);
      t.bits_per_block = 1000;
      CHECK(resolve(s, t, true).warm == 4096);
      t.bits_per_block = 0;
      CHECK(resolve(s, t, true).warm == 0);
    }
    s.sync_warm = "0";
    CHECK(resolve(s, t, true).warm == 0);
    s.sync_warm = "1000";  // taken as given: the launcher rounds and clamps
    CHECK(resolve(s, t, true).warm == 1000);
    s.sync_warm = "100000";
    CHECK(resolve(s, t, true).warm == 100000);
  }
  {  // chunks: a set, non-empty value decides; else spec || bits_per_block <= 128
    JpegSwitches s;
    s.sync = "pass";
    BatchTraits t = easy();
    for (const char *v : {(const char *)nullptr, ""}) {
      s.chunks = v;
      t.bits_per_block = 128;
      CHECK(resolve(s, t, true).chunks);
      t.bits_per_block = 129;
      CHECK(!resolve(s, t, true).chunks);
      JpegSwitches a = s;
      a.sync = "spec";  // after the speculative sync always
      CHECK(resolve(a, t, true).chunks);
    }
    s.chunks = "1";
    CHECK(resolve(s, t, true).chunks);
    s.chunks = "0";
    t.bits_per_block = 10;
    CHECK(!resolve(s, t, true).chunks);
    s.sync = "spec";
    CHECK(!resolve(s, t, true).chunks);
  }
  {  // write4, fuse, fuse_idct, stats, trace
    JpegSwitches s;
    BatchTraits t = easy();
    s.write4 = "0";
    CHECK(!resolve(s, t, true).write4);
    s.write4 = "1";
    CHECK(resolve(s, t, true).write4);
    s.fuse_idct = "0";
    CHECK(resolve(s, t, true).fuse && !resolve(s, t, true).fuse_idct);
    s.fuse_idct = "1";
    CHECK(resolve(s, t, true).fuse_idct && !resolve(s, t, false).fuse_idct);
    t.d422 = false;
    CHECK(resolve(s, t, true).fuse && !resolve(s, t, true).fuse_idct);
    t.d422 = true;
    s.fuse = "0";  // the pixel round trip: nothing to fuse the IDCT into
    CHECK(!resolve(s, t, true).fuse && !resolve(s, t, true).fuse_idct);
    s.sync_stats = "";
    s.trace = "0";  // set is on, whatever the value
    CHECK(resolve(s, t, true).stats && resolve(s, t, true).trace);
  }
  std::printf("{\"checks\": %d, \"failed\": %d}\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}

// dec_syncg instantiates (layout 0: G 1 2 3 4 8), (1: 4 5), (2: 4 5); G = 0 is the legacy loop
static bool instantiated(int g, int tabs) {
  if (g == 0) return true;
  if (tabs == 0) return g == 1 || g == 2 || g == 3 || g == 4 || g == 8;
  return (tabs == 1 || tabs == 2) && (g == 4 || g == 5);
}

static int exhaustive() {
  const char *gs[] = {nullptr, "-1", "0", "1", "2", "3", "4", "5", "6", "7", "8", "9"};
  const char *flags[] = {nullptr, "0", "1"};
  int cases = 0;
  for (const char *g : gs)
    for (const char *tabs4 : flags)
      for (const char *lsb : flags)
        for (int bt = 0; bt < 2; ++bt)
          for (int bp = 0; bp < 2; ++bp) {
            JpegSwitches s;
            s.sync_g = g;
            s.sync_tabs4 = tabs4;
            s.sync_lsb = lsb;
            BatchTraits t = easy();
            t.tabs4 = bt != 0;
            t.pow2bpm = bp != 0;
            const DecodePlan p = resolve(s, t, true);
            ++cases;
            CHECK(instantiated(p.g, p.tabs));
            CHECK(p.tabs == 0 || (t.tabs4 && !(tabs4 && !std::strcmp(tabs4, "0"))));  // four tables only where they fit
            CHECK(p.tabs != 2 || (t.pow2bpm && !(lsb && !std::strcmp(lsb, "0"))));   // the LSB lane only where it fits
          }
  std::printf("{\"cases\": %d, \"failed\": %d}\n", cases, g_failed);
  return g_failed ? 1 : 0;
}

static int read_env() {
  const JpegSwitches s = JpegSwitches::read();
  const struct { const char *name, *v; } all[] = {
      {"VF_JPEG_SYNC", s.sync}, {"VF_JPEG_SYNC_LSB", s.sync_lsb}, {"VF_JPEG_SYNC_TABS4", s.sync_tabs4},
      {"VF_JPEG_SYNC_G", s.sync_g}, {"VF_JPEG_SYNC_QUEUED", s.sync_queued}, {"VF_JPEG_SYNC_WARM", s.sync_warm},
      {"VF_JPEG_SYNC_STATS", s.sync_stats}, {"VF_JPEG_CHUNKS", s.chunks}, {"VF_JPEG_WRITE4", s.write4},
      {"VF_JPEG_FUSE", s.fuse}, {"VF_JPEG_FUSE_IDCT", s.fuse_idct}, {"VF_JPEG_IDCT24", s.idct24},
      {"VF_JPEG_FETCH_LEARN", s.fetch_learn}, {"VF_JPEG_TRACE", s.trace}};
  for (const auto &e : all) std::printf("%s=%s\n", e.name, e.v ? e.v : "<unset>");
  return 0;
}

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "rules") return rules();
  if (mode == "exhaustive") return exhaustive();
  if (mode == "read") return read_env();
  std::fprintf(stderr, "usage: %s rules | exhaustive | read\n", argv[0]);
  return 2;
}
