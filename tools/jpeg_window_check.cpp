// Host twin of the windowed pixel pass (tdeed_jpeg_pixels_window, t-deed_amd/csrc/jpeg.hip): the band loop of the kernel in
// plain loops over jc_window's ranges, no GPU, for running under host sanitizers.  Sibling of tools/jpeg_host_check.cpp.
//
//   c++ -O1 -g -std=c++17 -fsanitize=address,undefined -o jpeg_window_check tools/jpeg_window_check.cpp
//   jpeg_window_check packed.bin [top left wh ww]...
//
// packed.bin: a packed video written by tdeed_amd.jpegdev.PackedJpegs.save (see jpeg_host_check.cpp).  Without windows on
// the command line the grid of tests/test_resident_video_host.py runs: every left in 0..17, widths 1, 2, 15, 16, 17 and "to
// the right edge", tops 0, 1, 7, 8, 15, 16, heights 1, 9 and "to the bottom edge", as far as they fit the frame.
//
// Per frame and window:
//   * the frame's coefficients are copied into an exact-size heap block in which every block of an MCU row outside
//     jc_window's mrow range holds 0x7FFF (what an unlisted piece would have left is never read, or the pixels differ);
//   * per band the planes are exact-size heap blocks as wide as jc_window's block columns (a sample outside them is a
//     heap overflow the sanitizer reports), IDCT runs for the listed blocks only, and every sample jc_pixel reads must
//     have been written (a `written` map beside each plane; a miss ends the program with status 1);
//   * the window's pixels must equal the same pixels of the whole-frame decode.
// Prints one line of totals; status 0 when everything matched.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../t-deed_amd/csrc/jpeg_core.h"

struct FullPlanes {
  const uint8_t* p[3];
  int pitch[3];
  int at(int c, int row, int col) const { return p[c][(long)row * pitch[c] + col]; }
};

// the kernel's BandPlanes with a map of the samples phase 1 wrote
struct CheckedBandPlanes {
  const uint8_t* p[3];
  const uint8_t* written[3];
  int ypitch, cpitch, y0, c0, yx0, cx0;
  mutable long misses;
  int at(int c, int row, int col) const {
    const long i = c == 0 ? (long)(row - y0) * ypitch + col - yx0 : (long)(row - c0) * cpitch + col - cx0;
    if (!written[c][i]) ++misses;
    return p[c][i];
  }
};

template <int SAMP>
static void full_pixels(const JcGeom& g, const FullPlanes& P, uint8_t* out) {
  const long px = (long)g.H * g.W;
  for (int y = 0; y < g.H; ++y)
    for (int x = 0; x < g.W; ++x) {
      int r, gg, b;
      jc_pixel<SAMP>(P, x, y, g.cw[g.ncomp - 1], g.ch[g.ncomp - 1], r, gg, b);
      out[(long)y * g.W + x] = (uint8_t)r;
      out[px + (long)y * g.W + x] = (uint8_t)gg;
      out[2 * px + (long)y * g.W + x] = (uint8_t)b;
    }
}

static void put_rows(uint8_t* plane, uint8_t* mark, int pitch, int row0, int n_rows, int src_row0, const uint32_t* rows) {
  for (int r = 0; r < n_rows; ++r)
    for (int x = 0; x < 8; ++x) {
      plane[(long)(row0 + r) * pitch + x] = (uint8_t)(rows[2 * (src_row0 + r) + (x >> 2)] >> (8 * (x & 3)));
      mark[(long)(row0 + r) * pitch + x] = 1;
    }
}

// the kernel body for one frame: coefficients fc (16-byte aligned), window w -> out (3, wh, ww); returns the read misses
template <int SAMP>
static long window_pixels(const JcGeom& g, const JcWindow& w, const int16_t* fc, const JcTableSet* ts, uint8_t* out) {
  constexpr int HS = (SAMP == JC_422 || SAMP == JC_420) ? 2 : 1, VS = SAMP == JC_420 ? 2 : 1;
  constexpr int NC = SAMP == JC_GREY ? 0 : 2, HALO = SAMP == JC_420 ? 1 : 0, CROWS = 8 + 2 * HALO;
  const int mcus_x = g.mcus_x, mcus_y = g.mcus_y, bw0 = mcus_x * HS;
  const int ypitch = w.ybx_n * 8, cpitch = w.cbx_n * 8;
  const long luma_blocks = (long)bw0 * mcus_y * VS, chroma_blocks = (long)mcus_x * mcus_y;
  const long plane_px = (long)w.wh * w.ww;
  long misses = 0;
  for (int band = w.band_lo; band < w.band_lo + w.band_n; ++band) {
    std::vector<uint8_t> ly((long)8 * VS * ypitch), my(ly.size(), 0);
    std::vector<uint8_t> lc[2], mc[2];
    for (int c = 0; c < NC; ++c) {
      lc[c].assign((long)CROWS * cpitch, 0);
      mc[c].assign((long)CROWS * cpitch, 0);
    }
    uint32_t rows[16];
    for (int v = 0; v < VS; ++v)
      for (int bx = 0; bx < w.ybx_n; ++bx) {
        if (band * VS + v < w.ybr_lo || band * VS + v > w.ybr_hi) continue;
        jc_idct_block(fc + ((long)(band * VS + v) * bw0 + w.ybx_lo + bx) * 64, ts->quant[ts->tq[0] & 3], rows);
        put_rows(ly.data() + bx * 8, my.data() + bx * 8, ypitch, v * 8, 8, 0, rows);
      }
    for (int c = 0; c < NC; ++c)
      for (int rel = 0; rel < 1 + 2 * HALO; ++rel)
        for (int bx = 0; bx < w.cbx_n; ++bx) {
          const int by = band + rel - HALO;
          if (by < 0 || by >= mcus_y || by < w.mrow_lo || by > w.mrow_hi) continue;
          jc_idct_block(fc + (luma_blocks + c * chroma_blocks + (long)by * mcus_x + w.cbx_lo + bx) * 64,
                        ts->quant[ts->tq[1 + c] & 3], rows);
          uint8_t* plane = lc[c].data() + bx * 8;
          uint8_t* mark = mc[c].data() + bx * 8;
          if (HALO && rel == 0) put_rows(plane, mark, cpitch, 0, 1, 7, rows);
          else if (HALO && rel == 2) put_rows(plane, mark, cpitch, 9, 1, 0, rows);
          else put_rows(plane, mark, cpitch, HALO, 8, 0, rows);
        }
    CheckedBandPlanes P;
    P.p[0] = ly.data(); P.written[0] = my.data();
    for (int c = 0; c < 2; ++c) {
      P.p[1 + c] = NC ? lc[c].data() : nullptr;
      P.written[1 + c] = NC ? mc[c].data() : nullptr;
    }
    P.ypitch = ypitch; P.cpitch = cpitch;
    P.y0 = band * 8 * VS; P.c0 = band * 8 - HALO;
    P.yx0 = w.ybx_lo * 8; P.cx0 = w.cbx_lo * 8;
    P.misses = 0;
    const int cw = (g.W + HS - 1) / HS, ch = (g.H + VS - 1) / VS;
    const int y_lo = band * 8 * VS > w.top ? band * 8 * VS : w.top;
    const int y_end = (band + 1) * 8 * VS < w.top + w.wh ? (band + 1) * 8 * VS : w.top + w.wh;
    for (int y = y_lo; y < y_end; ++y)
      for (int i = 0; i < w.ww; ++i) {
        int r, gg, b;
        jc_pixel<SAMP>(P, w.left + i, y, cw, ch, r, gg, b);
        uint8_t* o = out + (long)(y - w.top) * w.ww + i;
        o[0] = (uint8_t)r;
        o[plane_px] = (uint8_t)gg;
        o[2 * plane_px] = (uint8_t)b;
      }
    misses += P.misses;
  }
  return misses;
}

static bool read_all(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc < 2 || (argc - 2) % 4 != 0) {
    fprintf(stderr, "usage: %s packed.bin [top left wh ww]...\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  int32_t hdr[8];
  if (!read_all(f, hdr, sizeof hdr) || hdr[0] != 0x314B504A) {
    fprintf(stderr, "%s: not a packed video\n", argv[1]);
    return 2;
  }
  const int W = hdr[1], H = hdr[2], samp = hdr[3], n_frames = hdr[4], n_seg = hdr[5], n_sets = hdr[6];
  const long stream_bytes = hdr[7];
  if (W <= 0 || H <= 0 || W > 65535 || H > 65535 || samp < JC_GREY || samp > JC_420 || n_frames < 0 || n_seg < 0 || n_sets < 0 ||
      stream_bytes < 0) {
    fprintf(stderr, "%s: bad header\n", argv[1]);
    return 2;
  }
  std::vector<int32_t> frame_set(n_frames);
  std::vector<JcSegment> segs(n_seg);
  std::vector<JcTableSet> sets(n_sets);
  std::vector<uint8_t> stream(stream_bytes);
  if (!read_all(f, frame_set.data(), sizeof(int32_t) * n_frames) || !read_all(f, segs.data(), sizeof(JcSegment) * n_seg) ||
      !read_all(f, sets.data(), sizeof(JcTableSet) * n_sets) || !read_all(f, stream.data(), stream_bytes)) {
    fprintf(stderr, "%s: truncated\n", argv[1]);
    return 2;
  }
  fclose(f);

  const JcGeom g = jc_geom(W, H, samp);
  const long frame_coefs = (long)g.frame_blocks * 64;
  std::vector<int16_t> coef_store(frame_coefs * n_frames + 8, 0);
  int16_t* coef = coef_store.data();
  while (((uintptr_t)coef) & 15) ++coef;
  for (int i = 0; i < n_seg; ++i) {
    const JcSegment& s = segs[i];
    if (!jc_segment_ok(s, stream_bytes, n_sets, g.mcus_x * g.mcus_y) || s.frame < 0 || s.frame >= n_frames) continue;
    jc_entropy_segment(stream.data() + s.offset, s.length, s.first_mcu, s.n_mcu, &sets[s.set], samp, g.mcus_x, g.mcus_y,
                       coef + (long)s.frame * frame_coefs);
  }

  std::vector<int> wins;                                   // top, left, wh, ww
  for (int a = 2; a + 3 < argc; a += 4) {
    const int top = atoi(argv[a]), left = atoi(argv[a + 1]), wh = atoi(argv[a + 2]), ww = atoi(argv[a + 3]);
    if (top < 0 || left < 0 || wh <= 0 || ww <= 0 || wh > H - top || ww > W - left) {
      fprintf(stderr, "window %dx%d at (%d, %d) is empty or leaves the %dx%d frame\n", wh, ww, top, left, H, W);
      return 2;
    }
    wins.insert(wins.end(), {top, left, wh, ww});
  }
  if (wins.empty()) {
    const int tops[] = {0, 1, 7, 8, 15, 16}, widths[] = {1, 2, 15, 16, 17, -1}, heights[] = {1, 9, -1};
    for (int top : tops)
      for (int hh : heights)
        for (int left = 0; left <= 17; ++left)
          for (int wd : widths) {
            const int wh = hh < 0 ? H - top : hh, ww = wd < 0 ? W - left : wd;
            if (top < H && left < W && wh > 0 && ww > 0 && wh <= H - top && ww <= W - left) wins.insert(wins.end(), {top, left, wh, ww});
          }
  }

  const long px = (long)H * W;
  std::vector<uint8_t> full(3 * px);
  std::vector<uint8_t> planes[3];
  for (int c = 0; c < g.ncomp; ++c) planes[c].resize((long)g.bw[c] * 8 * g.bh[c] * 8);
  long n_checked = 0, n_bad = 0, n_miss = 0;
  for (int fr = 0; fr < n_frames; ++fr) {
    const int set = frame_set[fr];
    if (set < 0 || set >= n_sets) continue;
    const int16_t* fc = coef + fr * frame_coefs;
    FullPlanes P;
    for (int c = 0; c < g.ncomp; ++c) {
      const int pitch = g.bw[c] * 8;
      for (int by = 0; by < g.bh[c]; ++by)
        for (int bx = 0; bx < g.bw[c]; ++bx) {
          uint32_t rows[16];
          jc_idct_block(fc + ((long)g.boff[c] + (long)by * g.bw[c] + bx) * 64, sets[set].quant[sets[set].tq[c] & 3], rows);
          for (int r = 0; r < 8; ++r)
            for (int x = 0; x < 8; ++x)
              planes[c][(long)(by * 8 + r) * pitch + bx * 8 + x] = (uint8_t)(rows[2 * r + (x >> 2)] >> (8 * (x & 3)));
        }
      P.p[c] = planes[c].data();
      P.pitch[c] = pitch;
    }
    switch (samp) {
      case JC_GREY: full_pixels<JC_GREY>(g, P, full.data()); break;
      case JC_444: full_pixels<JC_444>(g, P, full.data()); break;
      case JC_422: full_pixels<JC_422>(g, P, full.data()); break;
      default: full_pixels<JC_420>(g, P, full.data()); break;
    }
    for (size_t k = 0; k + 3 < wins.size(); k += 4) {
      const int top = wins[k], left = wins[k + 1], wh = wins[k + 2], ww = wins[k + 3];
      const JcWindow w = jc_window(g, top, left, wh, ww);
      // the frame's coefficients with every block of an MCU row outside [mrow_lo, mrow_hi] poisoned
      std::vector<int16_t> own_store(frame_coefs + 8);
      int16_t* own = own_store.data();
      while (((uintptr_t)own) & 15) ++own;
      memcpy(own, fc, sizeof(int16_t) * frame_coefs);
      for (int c = 0; c < g.ncomp; ++c) {
        const int v = c == 0 ? g.vs : 1;
        for (int by = 0; by < g.bh[c]; ++by)
          if (by / v < w.mrow_lo || by / v > w.mrow_hi)
            for (long i = 0; i < (long)g.bw[c] * 64; ++i) own[((long)g.boff[c] + (long)by * g.bw[c]) * 64 + i] = 0x7FFF;
      }
      std::vector<uint8_t> out(3L * wh * ww);
      long miss = 0;
      switch (samp) {
        case JC_GREY: miss = window_pixels<JC_GREY>(g, w, own, &sets[set], out.data()); break;
        case JC_444: miss = window_pixels<JC_444>(g, w, own, &sets[set], out.data()); break;
        case JC_422: miss = window_pixels<JC_422>(g, w, own, &sets[set], out.data()); break;
        default: miss = window_pixels<JC_420>(g, w, own, &sets[set], out.data()); break;
      }
      bool same = true;
      for (int c = 0; c < 3 && same; ++c)
        for (int y = 0; y < wh && same; ++y)
          same = memcmp(out.data() + ((long)c * wh + y) * ww, full.data() + c * px + (long)(top + y) * W + left, ww) == 0;
      ++n_checked;
      n_miss += miss;
      if (!same || miss) {
        ++n_bad;
        fprintf(stderr, "frame %d window %dx%d at (%d, %d): %s, %ld samples read that phase 1 did not write\n", fr, wh, ww, top,
                left, same ? "pixels equal" : "PIXELS DIFFER", miss);
      }
    }
  }
  printf("%ld frame windows checked, %ld wrong, %ld unwritten samples read\n", n_checked, n_bad, n_miss);
  return n_bad ? 1 : 0;
}
