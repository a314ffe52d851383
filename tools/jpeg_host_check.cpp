// Host twin of the device JPEG decoder: the per-segment and per-frame functions of t-deed_amd/csrc/jpeg_core.h in plain
// loops, no GPU.  Reads a packed video written by tdeed_amd.jpegdev.PackedJpegs.save and writes coefficients, statuses
// and RGB, so that the shared arithmetic and its behaviour on damaged streams can be checked (and run under host
// sanitizers) without a device.
//
//   c++ -O2 -std=c++17 -o jpeg_host_check tools/jpeg_host_check.cpp
//   jpeg_host_check packed.bin out.bin
//
// packed.bin: int32 header {magic 'JPK1', W, H, sampling, frames, segments, table sets, stream bytes}, int32
//   frame_set[frames], int32 segments[segments][6], table sets [sets][4240], stream bytes.
// out.bin: int16 coefficients [frames][frame_blocks * 64], int32 status[segments], uint8 rgb [frames][3][H][W]
//   (zero for a frame without a table set).
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

template <int SAMP>
static void frame_pixels(const JcGeom& g, const FullPlanes& P, uint8_t* out) {
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

static bool read_all(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s packed.bin out.bin\n", argv[0]);
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
  // 16-byte aligned rows for jc_idct_block: the vector's storage is over-allocated and the base rounded up
  std::vector<int16_t> coef_store(frame_coefs * n_frames + 8, 0);
  int16_t* coef = coef_store.data();
  while (((uintptr_t)coef) & 15) ++coef;
  std::vector<int32_t> status(n_seg, 0);
  for (int i = 0; i < n_seg; ++i) {
    const JcSegment& s = segs[i];
    if (!jc_segment_ok(s, stream_bytes, n_sets, g.mcus_x * g.mcus_y) || s.frame < 0 || s.frame >= n_frames) {
      status[i] = JC_ERR_TABLE;
      continue;
    }
    // the segment alone in an exact-size heap block: a read outside [offset, offset + length) is an error the sanitizer sees
    std::vector<uint8_t> own(stream.begin() + s.offset, stream.begin() + s.offset + s.length);
    status[i] = jc_entropy_segment(own.data(), s.length, s.first_mcu, s.n_mcu, &sets[s.set], samp, g.mcus_x, g.mcus_y,
                                   coef + (long)s.frame * frame_coefs);
  }

  const long px = (long)H * W;
  std::vector<uint8_t> rgb(3 * px * n_frames, 0);
  std::vector<uint8_t> planes[3];
  for (int c = 0; c < g.ncomp; ++c) planes[c].resize((long)g.bw[c] * 8 * g.bh[c] * 8);
  for (int fr = 0; fr < n_frames; ++fr) {
    const int set = frame_set[fr];
    if (set < 0 || set >= n_sets) continue;
    FullPlanes P;
    for (int c = 0; c < g.ncomp; ++c) {
      const int pitch = g.bw[c] * 8;
      for (int by = 0; by < g.bh[c]; ++by)
        for (int bx = 0; bx < g.bw[c]; ++bx) {
          uint32_t rows[16];
          jc_idct_block(coef + fr * frame_coefs + ((long)g.boff[c] + (long)by * g.bw[c] + bx) * 64,
                        sets[set].quant[sets[set].tq[c] & 3], rows);
          for (int r = 0; r < 8; ++r)
            for (int x = 0; x < 8; ++x)
              planes[c][(long)(by * 8 + r) * pitch + bx * 8 + x] = (uint8_t)(rows[2 * r + (x >> 2)] >> (8 * (x & 3)));
        }
      P.p[c] = planes[c].data();
      P.pitch[c] = pitch;
    }
    uint8_t* o = rgb.data() + 3 * px * fr;
    switch (samp) {
      case JC_GREY: frame_pixels<JC_GREY>(g, P, o); break;
      case JC_444: frame_pixels<JC_444>(g, P, o); break;
      case JC_422: frame_pixels<JC_422>(g, P, o); break;
      default: frame_pixels<JC_420>(g, P, o); break;
    }
  }

  FILE* o = fopen(argv[2], "wb");
  if (!o) {
    perror(argv[2]);
    return 2;
  }
  fwrite(coef, sizeof(int16_t), frame_coefs * n_frames, o);
  fwrite(status.data(), sizeof(int32_t), n_seg, o);
  fwrite(rgb.data(), 1, rgb.size(), o);
  fclose(o);
  int bad = 0;
  for (int i = 0; i < n_seg; ++i) bad += status[i] != 0;
  printf("%d frames, %d segments, %d table sets, %d segments with errors\n", n_frames, n_seg, n_sets, bad);
  return 0;
}
