// Whole-video scoring: clip windows gathered from a resident frame buffer, clip scores stitched into a per-video track.
#include "common.h"

// =========================================================================== clip gather
// clips_out[b][t] = video[starts[b] + t], a zero frame where the window hangs over either end of the video (the padding
// of the reference's FrameReaderVideo.load_frames(pad=True)).  blockIdx.y = frame slot b*T + t: one 32-bit division per
// workgroup, none per element.  A workgroup walks its share of the frame in 16-byte chunks.
__global__ __launch_bounds__(256) void clip_gather_v16_kernel(const u32x4* __restrict__ video, int L, long chunks,
                                                              const int* __restrict__ starts, int T,
                                                              u32x4* __restrict__ out) {
  const int slot = blockIdx.y;
  const int b = slot / T;
  const long f = (long)starts[b] + (slot - b * T);
  const bool real = f >= 0 && f < L;
  const u32x4* src = video + (real ? f : 0) * chunks;
  u32x4* dst = out + (long)slot * chunks;
  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < chunks; i += (long)gridDim.x * 256)
    dst[i] = real ? src[i] : zero;
}

// frame sizes that are no multiple of 16 bytes (or unaligned buffers)
__global__ __launch_bounds__(256) void clip_gather_u8_kernel(const uint8_t* __restrict__ video, int L, long frame_bytes,
                                                             const int* __restrict__ starts, int T,
                                                             uint8_t* __restrict__ out) {
  const int slot = blockIdx.y;
  const int b = slot / T;
  const long f = (long)starts[b] + (slot - b * T);
  const bool real = f >= 0 && f < L;
  const uint8_t* src = video + (real ? f : 0) * frame_bytes;
  uint8_t* dst = out + (long)slot * frame_bytes;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < frame_bytes; i += (long)gridDim.x * 256)
    dst[i] = real ? src[i] : (uint8_t)0;
}

extern "C" int tdeed_clip_gather_u8(const uint8_t* video, int L, long frame_bytes, const int* starts, int B, int T,
                                    uint8_t* clips_out, void* stream) {
  TD_CHECK(video && starts && clips_out, "clip_gather: null pointer");
  TD_CHECK(L > 0 && frame_bytes > 0 && B > 0 && T > 0, "clip_gather: bad sizes");
  TD_CHECK((long)B * T <= 65535, "clip_gather: B*T=%ld frame slots exceed the grid's 65535", (long)B * T);
  hipStream_t st = (hipStream_t)stream;
  const bool v16 = frame_bytes % 16 == 0 && (((uintptr_t)video | (uintptr_t)clips_out) & 15) == 0;
  if (v16) {
    const long chunks = frame_bytes / 16;
    const int gx = (int)(cdiv(chunks, 256 * 4) < 64 ? cdiv(chunks, 256 * 4) : 64);     // 4+ chunks per thread
    hipLaunchKernelGGL(clip_gather_v16_kernel, dim3(gx, B * T), dim3(256), 0, st, (const u32x4*)video, L, chunks, starts, T,
                       (u32x4*)clips_out);
  } else {
    const int gx = (int)(cdiv(frame_bytes, 256 * 4) < 64 ? cdiv(frame_bytes, 256 * 4) : 64);
    hipLaunchKernelGGL(clip_gather_u8_kernel, dim3(gx, B * T), dim3(256), 0, st, video, L, frame_bytes, starts, T, clips_out);
  }
  TD_LAUNCH_CHECK("clip_gather");
  return TDEED_OK;
}

// =========================================================================== score stitching
// Device twin of evalutil.ScoreStitcher (add / add_views / normalised).  One thread owns one video frame: it walks the
// clips in the order given and, per covering clip, adds the views one after the other -- the same sequence of fp32
// additions per frame as the host's clip-major loop, so sums, support and mean carry the same bits.  No atomics.
__global__ __launch_bounds__(256) void stitch_scores_kernel(const float* __restrict__ clip_scores, int V, int n, int T, int K1,
                                                            const int* __restrict__ starts, int count_all, int L,
                                                            float* __restrict__ track_sum, int* __restrict__ support,
                                                            float* __restrict__ mean_out) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= L) return;
  float* s = track_sum + (long)f * K1;
  int sup = support[f];
  for (int i = 0; i < n; ++i) {
    const long t = (long)f - starts[i];
    if (t < 0 || t >= T) continue;
    for (int v = 0; v < V; ++v) {
      const float* p = clip_scores + (((long)v * n + i) * T + t) * K1;
      bool nz = false;
      for (int k = 0; k < K1; ++k) {
        const float x = p[k];
        s[k] += x;
        nz |= x != 0.f;
      }
      sup += (count_all || nz) ? 1 : 0;
    }
  }
  support[f] = sup;
  if (mean_out) {
    const float d = (float)(sup > 1 ? sup : 1);
    for (int k = 0; k < K1; ++k) mean_out[(long)f * K1 + k] = s[k] / d;     // IEEE division (no fast-math in this build)
  }
}

extern "C" int tdeed_stitch_scores(const float* clip_scores, int V, int n, int T, int K1, const int* starts, int count_all,
                                   int L, float* track_sum, int* support, float* mean_out, void* stream) {
  TD_CHECK(clip_scores && starts && track_sum && support, "stitch_scores: null pointer");
  TD_CHECK(V > 0 && n > 0 && T > 0 && K1 > 0 && L > 0, "stitch_scores: bad sizes");
  TD_CHECK(count_all == 0 || count_all == 1, "stitch_scores: count_all must be 0 or 1");
  hipLaunchKernelGGL(stitch_scores_kernel, dim3(cdiv(L, 256)), dim3(256), 0, (hipStream_t)stream, clip_scores, V, n, T, K1,
                     starts, count_all, L, track_sum, support, mean_out);
  TD_LAUNCH_CHECK("stitch_scores");
  return TDEED_OK;
}
