// Baseline JPEG decode of a video's frames: entropy decode (one lane per segment) into an int16 coefficient buffer, then
// dequantisation, IDCT, up-sampling and colour conversion into the planar uint8 (n,3,H,W) layout of the resident-video
// consumers.  The arithmetic lives in jpeg_core.h (shared with tools/jpeg_host_check.cpp); tables and the packed stream
// come from tdeed_amd/jpegdev.py.
#include "common.h"
#include "jpeg_core.h"

// =========================================================================== entropy decode
// One wavefront per workgroup; waves[w] = (first row of the segment table, count <= 64).  The rows of a wavefront share
// one table set (jpegdev.PackedJpegs.waves), staged in LDS once.  Lane i decodes segment first + i: sequential inside
// the segment, one flat per-symbol loop (jc_entropy_segment), so lanes in different blocks re-converge every symbol.
// A lane reads only [offset, offset + length) of the stream and stores only inside its frame's coefficient range; a row
// that points outside the buffers, a frame outside [frame_lo, frame_lo + n_frames) or a foreign table set gets
// JC_ERR_TABLE and touches nothing.  status[row] = 0 or the JC_ERR_* code.
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const uint8_t* __restrict__ stream, long stream_bytes,
                                                          const JcSegment* __restrict__ segs, int n_segments,
                                                          const int* __restrict__ waves, const JcTableSet* __restrict__ sets,
                                                          int n_sets, int samp, int mcus_x, int mcus_y, int frame_lo, int n_frames,
                                                          long frame_coefs, int16_t* __restrict__ coef, int* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) JcTableSet ts;
  const int lane = threadIdx.x;
  int first = waves[2 * blockIdx.x], count = waves[2 * blockIdx.x + 1];
  if (first < 0 || first >= n_segments) return;
  count = count < 64 ? count : 64;
  count = count < n_segments - first ? count : n_segments - first;
  const int set = segs[first].set;
  if (set < 0 || set >= n_sets) {
    if (lane < count) status[first + lane] = JC_ERR_TABLE;
    return;
  }
  const u32x4* src = reinterpret_cast<const u32x4*>(sets + set);
  u32x4* dst = reinterpret_cast<u32x4*>(&ts);
  for (int i = lane; i < JC_TABLE_SET_BYTES / 16; i += 64) dst[i] = src[i];
  __syncthreads();
  if (lane >= count) return;
  const JcSegment s = segs[first + lane];
  const long f = (long)s.frame - frame_lo;
  if (!jc_segment_ok(s, stream_bytes, n_sets, mcus_x * mcus_y) || s.set != set || f < 0 || f >= n_frames) {
    status[first + lane] = JC_ERR_TABLE;
    return;
  }
  status[first + lane] =
      jc_entropy_segment(stream + s.offset, s.length, s.first_mcu, s.n_mcu, &ts, samp, mcus_x, mcus_y, coef + f * frame_coefs);
}

extern "C" int tdeed_jpeg_entropy(const uint8_t* stream, long stream_bytes, const int* segments, int n_segments, const int* waves,
                                  int n_waves, const uint8_t* table_sets, int n_sets, int W, int H, int sampling, int frame_lo,
                                  int n_frames, int16_t* coeff, int* status, void* hip_stream) {
  TD_CHECK(stream && segments && waves && table_sets && coeff && status, "jpeg_entropy: null pointer");
  TD_CHECK(stream_bytes > 0 && n_segments > 0 && n_waves > 0 && n_sets > 0 && n_frames > 0 && frame_lo >= 0,
           "jpeg_entropy: bad sizes");
  TD_CHECK(W > 0 && H > 0 && W <= 65535 && H <= 65535, "jpeg_entropy: bad frame size %dx%d", H, W);
  TD_CHECK(sampling >= JC_GREY && sampling <= JC_420, "jpeg_entropy: sampling %d (0 grey, 1 4:4:4, 2 4:2:2, 3 4:2:0)", sampling);
  TD_CHECK((((uintptr_t)table_sets) & 15) == 0 && (((uintptr_t)segments | (uintptr_t)waves | (uintptr_t)status) & 3) == 0 &&
               (((uintptr_t)coeff) & 15) == 0,
           "jpeg_entropy: table sets and coefficients must be 16-byte aligned, the tables 4-byte");
  const JcGeom g = jc_geom(W, H, sampling);
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(n_waves), dim3(64), 0, (hipStream_t)hip_stream, stream, stream_bytes,
                     (const JcSegment*)segments, n_segments, waves, (const JcTableSet*)table_sets, n_sets, sampling, g.mcus_x,
                     g.mcus_y, frame_lo, n_frames, (long)g.frame_blocks * 64, coeff, status);
  TD_LAUNCH_CHECK("jpeg_entropy");
  return TDEED_OK;
}

extern "C" long tdeed_jpeg_frame_coeffs(int W, int H, int sampling) {
  if (W <= 0 || H <= 0 || W > 65535 || H > 65535 || sampling < JC_GREY || sampling > JC_420) return -1;
  return (long)jc_geom(W, H, sampling).frame_blocks * 64;
}

// =========================================================================== pixels
// Workgroup (band, frame): one MCU row of the frame.  Phase 1: one thread per block runs dequantisation and both IDCT
// passes and writes the samples into LDS planes -- luma 8 VS rows, chroma 8 rows, and for 4:2:0 one chroma row above and
// below the band (the up-sampling taps reach one chroma sample across the MCU border), taken from a recomputed IDCT of
// the neighbouring band's chroma blocks.  Phase 2: one thread per 16 pixels of a row: triangle taps, colour conversion,
// three 16-byte stores (V16) or guarded byte stores.
// The frame lands in row dst_row[frame] of out when ROWS (tdeed_jpeg_pixels_rows: the frames of a clip batch go to rows
// i * T + t of the batch slot), in row frame otherwise; a row outside [0, out_rows) stores nothing.
struct BandPlanes {
  const uint8_t* y;
  const uint8_t* cb;
  const uint8_t* cr;
  int ypitch, cpitch, y0, c0;      // luma row y0 / chroma row c0 is row 0 of the LDS plane
  __device__ __forceinline__ int at(int c, int row, int col) const {
    return c == 0 ? y[(row - y0) * ypitch + col] : (c == 1 ? cb : cr)[(row - c0) * cpitch + col];
  }
};

template <int SAMP, bool V16, bool ROWS>
__global__ __launch_bounds__(256) void jpeg_pixels_kernel(const int16_t* __restrict__ coef, const int* __restrict__ frame_set,
                                                          const JcTableSet* __restrict__ sets, int n_sets, int frame_lo,
                                                          int W, int H, int mcus_x, int mcus_y, uint8_t* __restrict__ out,
                                                          const int* __restrict__ dst_row, long out_rows) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  constexpr int HS = (SAMP == JC_422 || SAMP == JC_420) ? 2 : 1, VS = SAMP == JC_420 ? 2 : 1;
  constexpr int NC = SAMP == JC_GREY ? 0 : 2;                 // chroma planes
  constexpr int HALO = SAMP == JC_420 ? 1 : 0;
  constexpr int CROWS = 8 + 2 * HALO;
  const int band = blockIdx.x, fl = blockIdx.y;
  const int set = frame_set[frame_lo + fl];
  if (set < 0 || set >= n_sets) return;                        // a frame that is decoded on the host
  const long row = ROWS ? (long)dst_row[frame_lo + fl] : (long)frame_lo + fl;
  if (ROWS && (row < 0 || row >= out_rows)) return;            // a frame that no row of the slot takes
  TD_DEV_ASSERT(row >= 0 && (!ROWS || row < out_rows));
  const JcTableSet* ts = sets + set;
  const int bw0 = mcus_x * HS, ypitch = bw0 * 8, cpitch = mcus_x * 8;
  uint8_t* ly = lds;
  uint8_t* lc = lds + 8 * VS * ypitch;                         // [NC][CROWS][cpitch]
  const long luma_blocks = (long)bw0 * mcus_y * VS, chroma_blocks = (long)mcus_x * mcus_y;
  const int16_t* fc = coef + (long)fl * (luma_blocks + NC * chroma_blocks) * 64;

  const int nY = VS * bw0, crows_b = 1 + 2 * HALO, nC = NC * crows_b * mcus_x;
  for (int t = threadIdx.x; t < nY + nC; t += 256) {
    uint32_t rows[16];
    if (t < nY) {
      const int v = t / bw0, bx = t - v * bw0;
      jc_idct_block(fc + ((long)(band * VS + v) * bw0 + bx) * 64, ts->quant[ts->tq[0] & 3], rows);
#pragma unroll
      for (int r = 0; r < 8; ++r)
        *reinterpret_cast<u32x2*>(ly + (v * 8 + r) * ypitch + bx * 8) = (u32x2){rows[2 * r], rows[2 * r + 1]};
    } else {
      const int u = t - nY, per = crows_b * mcus_x;
      const int c = u / per, w = u - c * per, rel = w / mcus_x, bx = w - rel * mcus_x;
      const int by = band + rel - HALO;                        // rel 0 / 2 of 4:2:0: the band above / below
      if (by < 0 || by >= mcus_y) continue;
      jc_idct_block(fc + (luma_blocks + c * chroma_blocks + (long)by * mcus_x + bx) * 64, ts->quant[ts->tq[1 + c] & 3], rows);
      uint8_t* plane = lc + c * CROWS * cpitch + bx * 8;
      if (HALO && rel == 0) {
        *reinterpret_cast<u32x2*>(plane) = (u32x2){rows[14], rows[15]};
      } else if (HALO && rel == 2) {
        *reinterpret_cast<u32x2*>(plane + 9 * cpitch) = (u32x2){rows[0], rows[1]};
      } else {
#pragma unroll
        for (int r = 0; r < 8; ++r)
          *reinterpret_cast<u32x2*>(plane + (HALO + r) * cpitch) = (u32x2){rows[2 * r], rows[2 * r + 1]};
      }
    }
  }
  __syncthreads();

  BandPlanes P;
  P.y = ly; P.cb = lc; P.cr = lc + CROWS * cpitch;
  P.ypitch = ypitch; P.cpitch = cpitch;
  P.y0 = band * 8 * VS; P.c0 = band * 8 - HALO;
  const int cw = (W + HS - 1) / HS, ch = (H + VS - 1) / VS;
  const int y_lo = band * 8 * VS, rows_here = H - y_lo < 8 * VS ? H - y_lo : 8 * VS;
  const int chunks = (W + 15) / 16;
  const long plane_px = (long)H * W;
  uint8_t* of = out + row * 3 * plane_px;
  for (int t = threadIdx.x; t < rows_here * chunks; t += 256) {
    const int ry = t / chunks, x0 = (t - ry * chunks) * 16, y = y_lo + ry;
    uint32_t pr[4] = {0, 0, 0, 0}, pg[4] = {0, 0, 0, 0}, pb[4] = {0, 0, 0, 0};
    uint8_t* o = of + (long)y * W + x0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int x = x0 + i;
      if (V16 || x < W) {
        int r, g, b;
        jc_pixel<SAMP>(P, x, y, cw, ch, r, g, b);
        if (V16) {
          pr[i >> 2] |= (uint32_t)r << (8 * (i & 3));
          pg[i >> 2] |= (uint32_t)g << (8 * (i & 3));
          pb[i >> 2] |= (uint32_t)b << (8 * (i & 3));
        } else {
          o[i] = (uint8_t)r;
          o[plane_px + i] = (uint8_t)g;
          o[2 * plane_px + i] = (uint8_t)b;
        }
      }
    }
    if (V16) {
      *reinterpret_cast<u32x4*>(o) = (u32x4){pr[0], pr[1], pr[2], pr[3]};
      *reinterpret_cast<u32x4*>(o + plane_px) = (u32x4){pg[0], pg[1], pg[2], pg[3]};
      *reinterpret_cast<u32x4*>(o + 2 * plane_px) = (u32x4){pb[0], pb[1], pb[2], pb[3]};
    }
  }
}

// dst_row == nullptr: the identity-row instance (tdeed_jpeg_pixels)
template <int SAMP>
static int jpeg_pixels_launch(const int16_t* coef, const int* frame_set, const uint8_t* sets, int n_sets, uint8_t* out,
                              const int* dst_row, long out_rows, int frame_lo, int n_frames, int H, int W, hipStream_t st) {
  const JcGeom g = jc_geom(W, H, SAMP);
  const int halo = SAMP == JC_420 ? 1 : 0, nc = SAMP == JC_GREY ? 0 : 2;
  const long lds = 8L * g.vs * g.bw[0] * 8 + (long)nc * (8 + 2 * halo) * g.mcus_x * 8;
  TD_CHECK(lds <= 64 * 1024, "jpeg_pixels: a band of a %d pixel wide frame needs %ld bytes of LDS (limit 65536)", W, lds);
  TD_CHECK(g.mcus_y <= 65535 && n_frames <= 65535, "jpeg_pixels: %d bands x %d frames exceed the grid", g.mcus_y, n_frames);
  const bool v16 = W % 16 == 0 && (((uintptr_t)out) & 15) == 0;
  const dim3 grid(g.mcus_y, n_frames);
#define JPEG_PIXELS_GO(V16, ROWS)                                                                                              \
  hipLaunchKernelGGL((jpeg_pixels_kernel<SAMP, V16, ROWS>), grid, dim3(256), lds, st, coef, frame_set, (const JcTableSet*)sets, \
                     n_sets, frame_lo, W, H, g.mcus_x, g.mcus_y, out, dst_row, out_rows)
  if (dst_row) {
    if (v16) JPEG_PIXELS_GO(true, true); else JPEG_PIXELS_GO(false, true);
  } else {
    if (v16) JPEG_PIXELS_GO(true, false); else JPEG_PIXELS_GO(false, false);
  }
#undef JPEG_PIXELS_GO
  TD_LAUNCH_CHECK("jpeg_pixels");
  return TDEED_OK;
}

static int jpeg_pixels_any(const int16_t* coeff, const int* frame_table_set, const uint8_t* table_sets, int n_sets, uint8_t* out,
                           const int* dst_row, long out_rows, int frame_lo, int n_frames, int H, int W, int sampling,
                           void* hip_stream) {
  TD_CHECK(coeff && frame_table_set && table_sets && out, "jpeg_pixels: null pointer");
  TD_CHECK(n_sets > 0 && n_frames > 0 && frame_lo >= 0, "jpeg_pixels: bad sizes");
  TD_CHECK(W > 0 && H > 0 && W <= 65535 && H <= 65535, "jpeg_pixels: bad frame size %dx%d", H, W);
  TD_CHECK((((uintptr_t)table_sets | (uintptr_t)coeff) & 15) == 0 && (((uintptr_t)frame_table_set) & 3) == 0,
           "jpeg_pixels: table sets and coefficients must be 16-byte aligned");
  hipStream_t st = (hipStream_t)hip_stream;
  switch (sampling) {
    case JC_GREY:
      return jpeg_pixels_launch<JC_GREY>(coeff, frame_table_set, table_sets, n_sets, out, dst_row, out_rows, frame_lo, n_frames, H, W, st);
    case JC_444:
      return jpeg_pixels_launch<JC_444>(coeff, frame_table_set, table_sets, n_sets, out, dst_row, out_rows, frame_lo, n_frames, H, W, st);
    case JC_422:
      return jpeg_pixels_launch<JC_422>(coeff, frame_table_set, table_sets, n_sets, out, dst_row, out_rows, frame_lo, n_frames, H, W, st);
    case JC_420:
      return jpeg_pixels_launch<JC_420>(coeff, frame_table_set, table_sets, n_sets, out, dst_row, out_rows, frame_lo, n_frames, H, W, st);
  }
  TD_CHECK(false, "jpeg_pixels: sampling %d (0 grey, 1 4:4:4, 2 4:2:2, 3 4:2:0)", sampling);
  return TDEED_OK;
}

extern "C" int tdeed_jpeg_pixels(const int16_t* coeff, const int* frame_table_set, const uint8_t* table_sets, int n_sets,
                                 uint8_t* out, int frame_lo, int n_frames, int H, int W, int sampling, void* hip_stream) {
  return jpeg_pixels_any(coeff, frame_table_set, table_sets, n_sets, out, nullptr, 0, frame_lo, n_frames, H, W, sampling, hip_stream);
}

extern "C" int tdeed_jpeg_pixels_rows(const int16_t* coeff, const int* frame_table_set, const uint8_t* table_sets, int n_sets,
                                      uint8_t* out, long out_rows, const int* dst_row, int frame_lo, int n_frames, int H, int W,
                                      int sampling, void* hip_stream) {
  TD_CHECK(dst_row && (((uintptr_t)dst_row) & 3) == 0, "jpeg_pixels_rows: dst_row must be a 4-byte aligned device pointer");
  TD_CHECK(out_rows > 0, "jpeg_pixels_rows: out_rows %ld", out_rows);
  return jpeg_pixels_any(coeff, frame_table_set, table_sets, n_sets, out, dst_row, out_rows, frame_lo, n_frames, H, W, sampling,
                         hip_stream);
}
