// Whole-video scoring: clip windows gathered from a resident frame buffer, clip scores stitched into a per-video track.
#include "common.h"

// =========================================================================== clip gather
// clips_out[b][t] = video[starts[b] + t], a zero frame where the window hangs over either end of the video (the padding
// of the reference's FrameReaderVideo.load_frames(pad=True)).  blockIdx.y = frame slot b*T + t: one 32-bit division per
// workgroup, none per element.  A workgroup walks its share of the frame in 16-byte chunks.
// SEG: `video` packs several videos one after the other; clip b belongs to the video whose first packed frame is
// clip_base[b] and whose length is clip_len_v[b], starts[b] is local to it, and the window is cut at THAT video's ends (a
// window hanging over the end of video v must not read the first frames of video v+1).  L is then the packed total, and a
// table entry that points outside it yields a zero frame.
template <bool SEG>
__device__ __forceinline__ long clip_gather_source(int L, const int* __restrict__ starts, const int* __restrict__ clip_base,
                                                   const int* __restrict__ clip_len_v, int T, int slot) {
  const int b = slot / T;
  const long f = (long)starts[b] + (slot - b * T);
  if (!SEG) return f >= 0 && f < L ? f : -1;
  const long base = clip_base[b];
  const long p = base + f;
  return f >= 0 && f < clip_len_v[b] && base >= 0 && p < L ? p : -1;
}

// RING: `video` holds only ring_frames rows of the (virtual) buffer of L frames, frame p in row p % ring_frames -- the frame
// ring of a video longer than the device budget (feeder.RingUpload).  Which frame a slot reads, and whether it is padding,
// is decided as for the whole buffer; only the row differs.  The slot is uniform over the workgroup: one 32-bit remainder
// per workgroup, scalar.  Which rows are live the kernel cannot know: T <= ring_frames and the upload order are the caller's.
template <bool RING>
__device__ __forceinline__ long clip_gather_row(long f, int ring_frames) {
  if (f < 0) return 0;
  return RING ? (long)((unsigned)f % (unsigned)ring_frames) : f;
}

template <bool SEG, bool RING>
__global__ __launch_bounds__(256) void clip_gather_v16_kernel(const u32x4* __restrict__ video, int L, int ring_frames, long chunks,
                                                              const int* __restrict__ starts, const int* __restrict__ clip_base,
                                                              const int* __restrict__ clip_len_v, int T,
                                                              u32x4* __restrict__ out) {
  const int slot = blockIdx.y;
  const long f = clip_gather_source<SEG>(L, starts, clip_base, clip_len_v, T, slot);
  const bool real = f >= 0;
  const u32x4* src = video + clip_gather_row<RING>(f, ring_frames) * chunks;
  u32x4* dst = out + (long)slot * chunks;
  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < chunks; i += (long)gridDim.x * 256)
    dst[i] = real ? src[i] : zero;
}

// frame sizes that are no multiple of 16 bytes (or unaligned buffers)
template <bool SEG, bool RING>
__global__ __launch_bounds__(256) void clip_gather_u8_kernel(const uint8_t* __restrict__ video, int L, int ring_frames,
                                                             long frame_bytes, const int* __restrict__ starts,
                                                             const int* __restrict__ clip_base,
                                                             const int* __restrict__ clip_len_v, int T,
                                                             uint8_t* __restrict__ out) {
  const int slot = blockIdx.y;
  const long f = clip_gather_source<SEG>(L, starts, clip_base, clip_len_v, T, slot);
  const bool real = f >= 0;
  const uint8_t* src = video + clip_gather_row<RING>(f, ring_frames) * frame_bytes;
  uint8_t* dst = out + (long)slot * frame_bytes;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < frame_bytes; i += (long)gridDim.x * 256)
    dst[i] = real ? src[i] : (uint8_t)0;
}

template <bool SEG, bool RING = false>
static int clip_gather_launch(const uint8_t* video, int L, long frame_bytes, const int* starts, const int* clip_base,
                              const int* clip_len_v, int B, int T, uint8_t* clips_out, void* stream, int ring_frames = 0) {
  hipStream_t st = (hipStream_t)stream;
  const bool v16 = frame_bytes % 16 == 0 && (((uintptr_t)video | (uintptr_t)clips_out) & 15) == 0;
  if (v16) {
    const long chunks = frame_bytes / 16;
    const int gx = (int)(cdiv(chunks, 256 * 4) < 64 ? cdiv(chunks, 256 * 4) : 64);     // 4+ chunks per thread
    hipLaunchKernelGGL((clip_gather_v16_kernel<SEG, RING>), dim3(gx, B * T), dim3(256), 0, st, (const u32x4*)video, L, ring_frames,
                       chunks, starts, clip_base, clip_len_v, T, (u32x4*)clips_out);
  } else {
    const int gx = (int)(cdiv(frame_bytes, 256 * 4) < 64 ? cdiv(frame_bytes, 256 * 4) : 64);
    hipLaunchKernelGGL((clip_gather_u8_kernel<SEG, RING>), dim3(gx, B * T), dim3(256), 0, st, video, L, ring_frames, frame_bytes,
                       starts, clip_base, clip_len_v, T, clips_out);
  }
  TD_LAUNCH_CHECK("clip_gather");
  return TDEED_OK;
}

extern "C" int tdeed_clip_gather_u8(const uint8_t* video, int L, long frame_bytes, const int* starts, int B, int T,
                                    uint8_t* clips_out, void* stream) {
  TD_CHECK(video && starts && clips_out, "clip_gather: null pointer");
  TD_CHECK(L > 0 && frame_bytes > 0 && B > 0 && T > 0, "clip_gather: bad sizes");
  TD_CHECK((long)B * T <= 65535, "clip_gather: B*T=%ld frame slots exceed the grid's 65535", (long)B * T);
  return clip_gather_launch<false>(video, L, frame_bytes, starts, nullptr, nullptr, B, T, clips_out, stream);
}

extern "C" int tdeed_clip_gather_seg_u8(const uint8_t* video, int L_total, long frame_bytes, const int* starts,
                                        const int* clip_base, const int* clip_len_v, int B, int T, uint8_t* clips_out,
                                        void* stream) {
  TD_CHECK(video && starts && clip_base && clip_len_v && clips_out, "clip_gather_seg: null pointer");
  TD_CHECK(L_total > 0 && frame_bytes > 0 && B > 0 && T > 0, "clip_gather_seg: bad sizes");
  TD_CHECK((long)B * T <= 65535, "clip_gather_seg: B*T=%ld frame slots exceed the grid's 65535", (long)B * T);
  return clip_gather_launch<true>(video, L_total, frame_bytes, starts, clip_base, clip_len_v, B, T, clips_out, stream);
}

extern "C" int tdeed_clip_gather_ring_u8(const uint8_t* ring, int ring_frames, int L_total, long frame_bytes, const int* starts,
                                         const int* clip_base, const int* clip_len_v, int B, int T, uint8_t* clips_out,
                                         void* stream) {
  TD_CHECK(ring && starts && clip_base && clip_len_v && clips_out, "clip_gather_ring: null pointer");
  TD_CHECK(ring_frames > 0 && L_total > 0 && frame_bytes > 0 && B > 0 && T > 0, "clip_gather_ring: bad sizes");
  TD_CHECK((long)B * T <= 65535, "clip_gather_ring: B*T=%ld frame slots exceed the grid's 65535", (long)B * T);
  return clip_gather_launch<true, true>(ring, L_total, frame_bytes, starts, clip_base, clip_len_v, B, T, clips_out, stream,
                                        ring_frames);
}

// =========================================================================== row gather (per-frame trunk maps)
// out[b][t] = maps[starts[b] + t]: the clip gather over a resident buffer of per-frame ROWS of any type (the trunk map of every
// frame, computed once), with one difference: a frame outside its video copies row `pad_row` instead of zeros -- the map of
// a black frame is not zero.  L (L_total for SEG) rows are frames, rows >= L belong to the caller (pad_row is one of them).
template <bool SEG>
__global__ __launch_bounds__(256) void rows_gather_v16_kernel(const u32x4* __restrict__ maps, int L, long chunks, int pad_row,
                                                              const int* __restrict__ starts, const int* __restrict__ clip_base,
                                                              const int* __restrict__ clip_len_v, int T,
                                                              u32x4* __restrict__ out) {
  const int slot = blockIdx.y;
  const long f = clip_gather_source<SEG>(L, starts, clip_base, clip_len_v, T, slot);
  const u32x4* src = maps + (f >= 0 ? f : (long)pad_row) * chunks;
  u32x4* dst = out + (long)slot * chunks;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < chunks; i += (long)gridDim.x * 256) dst[i] = src[i];
}

// row sizes that are no multiple of 16 bytes (or unaligned buffers)
template <bool SEG>
__global__ __launch_bounds__(256) void rows_gather_u8_kernel(const uint8_t* __restrict__ maps, int L, long row_bytes, int pad_row,
                                                             const int* __restrict__ starts, const int* __restrict__ clip_base,
                                                             const int* __restrict__ clip_len_v, int T,
                                                             uint8_t* __restrict__ out) {
  const int slot = blockIdx.y;
  const long f = clip_gather_source<SEG>(L, starts, clip_base, clip_len_v, T, slot);
  const uint8_t* src = maps + (f >= 0 ? f : (long)pad_row) * row_bytes;
  uint8_t* dst = out + (long)slot * row_bytes;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < row_bytes; i += (long)gridDim.x * 256) dst[i] = src[i];
}

template <bool SEG>
static int rows_gather_launch(const uint8_t* maps, int L, long row_bytes, int pad_row, const int* starts, const int* clip_base,
                              const int* clip_len_v, int B, int T, uint8_t* out, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const bool v16 = row_bytes % 16 == 0 && (((uintptr_t)maps | (uintptr_t)out) & 15) == 0;
  if (v16) {
    const long chunks = row_bytes / 16;
    const int gx = (int)(cdiv(chunks, 256 * 4) < 64 ? cdiv(chunks, 256 * 4) : 64);     // 4+ chunks per thread
    hipLaunchKernelGGL(rows_gather_v16_kernel<SEG>, dim3(gx, B * T), dim3(256), 0, st, (const u32x4*)maps, L, chunks, pad_row,
                       starts, clip_base, clip_len_v, T, (u32x4*)out);
  } else {
    const int gx = (int)(cdiv(row_bytes, 256 * 4) < 64 ? cdiv(row_bytes, 256 * 4) : 64);
    hipLaunchKernelGGL(rows_gather_u8_kernel<SEG>, dim3(gx, B * T), dim3(256), 0, st, maps, L, row_bytes, pad_row, starts,
                       clip_base, clip_len_v, T, out);
  }
  TD_LAUNCH_CHECK("rows_gather");
  return TDEED_OK;
}

extern "C" int tdeed_rows_gather(const void* maps, int rows, long row_bytes, int L, int pad_row, const int* starts, int B, int T,
                                 void* out, void* stream) {
  TD_CHECK(maps && starts && out, "rows_gather: null pointer");
  TD_CHECK(rows > 0 && row_bytes > 0 && L > 0 && B > 0 && T > 0, "rows_gather: bad sizes");
  TD_CHECK(L <= rows && pad_row >= 0 && pad_row < rows, "rows_gather: L=%d frames and pad_row=%d must lie inside the %d rows", L,
           pad_row, rows);
  TD_CHECK((long)B * T <= 65535, "rows_gather: B*T=%ld row slots exceed the grid's 65535", (long)B * T);
  return rows_gather_launch<false>((const uint8_t*)maps, L, row_bytes, pad_row, starts, nullptr, nullptr, B, T, (uint8_t*)out,
                                   stream);
}

extern "C" int tdeed_rows_gather_seg(const void* maps, int rows, long row_bytes, int L_total, int pad_row, const int* starts,
                                     const int* clip_base, const int* clip_len_v, int B, int T, void* out, void* stream) {
  TD_CHECK(maps && starts && clip_base && clip_len_v && out, "rows_gather_seg: null pointer");
  TD_CHECK(rows > 0 && row_bytes > 0 && L_total > 0 && B > 0 && T > 0, "rows_gather_seg: bad sizes");
  TD_CHECK(L_total <= rows && pad_row >= 0 && pad_row < rows,
           "rows_gather_seg: L_total=%d frames and pad_row=%d must lie inside the %d rows", L_total, pad_row, rows);
  TD_CHECK((long)B * T <= 65535, "rows_gather_seg: B*T=%ld row slots exceed the grid's 65535", (long)B * T);
  return rows_gather_launch<true>((const uint8_t*)maps, L_total, row_bytes, pad_row, starts, clip_base, clip_len_v, B, T,
                                  (uint8_t*)out, stream);
}

// =========================================================================== score stitching
// Device twin of evalutil.ScoreStitcher (add / add_views / normalised).  One thread owns one video frame: it walks the
// clips in the order given and, per covering clip, adds the views one after the other -- the same sequence of fp32
// additions per frame as the host's clip-major loop, so sums, support and mean carry the same bits.  No atomics.
// f: the frame inside its video; s / support / mean_out: the frame's own row; the clips i0 .. i1 - 1 of the n are walked.
__device__ __forceinline__ void stitch_frame(const float* __restrict__ clip_scores, int V, int n, int T, int K1,
                                             const int* __restrict__ starts, int i0, int i1, int count_all, int f,
                                             float* __restrict__ s, int* __restrict__ support, float* __restrict__ mean_out) {
  int sup = *support;
  for (int i = i0; i < i1; ++i) {
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
  *support = sup;
  if (mean_out) {
    const float d = (float)(sup > 1 ? sup : 1);
    for (int k = 0; k < K1; ++k) mean_out[k] = s[k] / d;     // IEEE division (no fast-math in this build)
  }
}

// nv videos packed one after the other (evalutil.group_clip_table; one video: nv = 1): one thread per packed frame p.  It
// finds its video v (seg_off[v] <= p < seg_off[v+1], a binary search over the nv + 1 offsets) and walks only that video's
// clips clip_off[v] .. clip_off[v+1] - 1, in the order given: per frame the additions of ScoreStitcher on that video alone.
__global__ __launch_bounds__(256) void stitch_scores_seg_kernel(const float* __restrict__ clip_scores, int V, int n, int T, int K1,
                                                                const int* __restrict__ starts, const int* __restrict__ seg_off,
                                                                const int* __restrict__ clip_off, int nv, int count_all, int L,
                                                                float* __restrict__ track_sum, int* __restrict__ support,
                                                                float* __restrict__ mean_out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= L) return;
  int lo = 0, hi = nv;                                         // seg_off[lo] <= p < seg_off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (seg_off[mid] <= p) lo = mid; else hi = mid;
  }
  const int f = p - seg_off[lo];
  int i0 = clip_off[lo], i1 = clip_off[lo + 1];
  i0 = i0 > 0 ? i0 : 0;                                        // a table entry outside the clip list reads nothing
  i1 = i1 < n ? i1 : n;
  TD_DEV_ASSERT(f >= 0 && p < seg_off[lo + 1]);
  stitch_frame(clip_scores, V, n, T, K1, starts, i0, i1, count_all, f, track_sum + (long)p * K1, support + p,
               mean_out ? mean_out + (long)p * K1 : nullptr);
}

extern "C" int tdeed_stitch_scores_seg(const float* clip_scores, int V, int n, int T, int K1, const int* starts, const int* seg_off,
                                       const int* clip_off, int nv, int count_all, int L_total, float* track_sum, int* support,
                                       float* mean_out, void* stream) {
  TD_CHECK(clip_scores && starts && seg_off && clip_off && track_sum && support, "stitch_scores_seg: null pointer");
  TD_CHECK(V > 0 && n > 0 && T > 0 && K1 > 0 && L_total > 0 && nv > 0, "stitch_scores_seg: bad sizes");
  TD_CHECK(nv <= 65535, "stitch_scores_seg: %d videos in one group, at most 65535", nv);
  TD_CHECK(count_all == 0 || count_all == 1, "stitch_scores_seg: count_all must be 0 or 1");
  hipLaunchKernelGGL(stitch_scores_seg_kernel, dim3(cdiv(L_total, 256)), dim3(256), 0, (hipStream_t)stream, clip_scores, V, n, T,
                     K1, starts, seg_off, clip_off, nv, count_all, L_total, track_sum, support, mean_out);
  TD_LAUNCH_CHECK("stitch_scores_seg");
  return TDEED_OK;
}

// =========================================================================== live stitching
// stitch_scores_seg for a stream whose length is not known yet: one launch per BATCH of clips, the partial sums carried
// between launches in a ring -- ring_sum fp32 [R][K1], ring_sup int32 [R], frame p in row p % R.  One thread per frame p in
// [lo, hi), hi = min(limit, max(final_hi, starts[B-1] + T)): the rows that become final with this launch and the rows the
// batch touches.  The thread runs stitch_frame over the batch's clips on its ring row -- over the launches of a stream the
// additions stitch_scores_seg_kernel performs over the whole clip list, in its order, each partial sum stored as the fp32
// it is -- and, when p < final_hi (no later clip covers p), writes the row out at p - lo and zeroes the ring row for frame
// p + R.  The caller's duties: clips ascending over the launches, no clip of this batch covers a frame below lo, and
// hi - lo <= R (the rows of one launch are distinct).  No atomics, no LDS.
__global__ __launch_bounds__(256) void stitch_live_kernel(const float* __restrict__ clip_scores, int V, int B, int T, int K1,
                                                          const int* __restrict__ starts, int count_all, int lo, int final_hi,
                                                          int limit, int R, float* __restrict__ ring_sum,
                                                          int* __restrict__ ring_sup, float* __restrict__ out_sum,
                                                          int* __restrict__ out_sup, float* __restrict__ out_mean) {
  const long touch = B > 0 ? (long)starts[B - 1] + T : 0;     // one past the last frame the batch touches
  long hi = touch > final_hi ? touch : final_hi;
  hi = hi < limit ? hi : limit;
  const long pl = (long)lo + (long)blockIdx.x * 256 + threadIdx.x;
  if (pl >= hi) return;
  TD_DEV_ASSERT(hi - lo <= R);
  TD_DEV_ASSERT(B == 0 || lo == 0 || starts[0] >= lo);
  const int p = (int)pl;
  const unsigned row = (unsigned)p % (unsigned)R;
  const bool fin = p < final_hi;
  float* s = ring_sum + (long)row * K1;
  int* sup = ring_sup + row;
  const long o = (long)(p - lo);
  stitch_frame(clip_scores, V, B, T, K1, starts, 0, B, count_all, p, s, sup, fin && out_mean ? out_mean + o * K1 : nullptr);
  if (!fin) return;
  for (int k = 0; k < K1; ++k) {
    out_sum[o * K1 + k] = s[k];
    s[k] = 0.f;
  }
  out_sup[o] = *sup;
  *sup = 0;
}

extern "C" int tdeed_stitch_live(const float* clip_scores, int V, int B, int T, int K1, const int* starts, int count_all, int lo,
                                 int final_hi, int limit, int ring_rows, float* ring_sum, int* ring_sup, float* out_sum,
                                 int* out_sup, float* out_mean, void* stream) {
  TD_CHECK(ring_sum && ring_sup, "stitch_live: null pointer");
  TD_CHECK(V > 0 && B >= 0 && T > 0 && K1 > 0 && ring_rows > 0, "stitch_live: bad sizes");
  TD_CHECK(B == 0 || (clip_scores && starts), "stitch_live: a batch of %d clips without scores or starts", B);
  TD_CHECK(count_all == 0 || count_all == 1, "stitch_live: count_all must be 0 or 1");
  TD_CHECK(0 <= lo && lo <= final_hi && final_hi <= limit, "stitch_live: rows [%d, %d) become final of %d frames", lo, final_hi,
           limit);
  TD_CHECK(final_hi - lo <= ring_rows, "stitch_live: %d rows become final, the ring holds %d", final_hi - lo, ring_rows);
  TD_CHECK(final_hi == lo || (out_sum && out_sup), "stitch_live: rows become final and there is nowhere to write them");
  const long rows = (long)limit - lo < ring_rows ? (long)limit - lo : ring_rows;      // no launch touches more
  if (rows <= 0) return TDEED_OK;
  hipLaunchKernelGGL(stitch_live_kernel, dim3((unsigned)cdiv(rows, 256)), dim3(256), 0, (hipStream_t)stream, clip_scores, V, B, T,
                     K1, starts, count_all, lo, final_hi, limit, ring_rows, ring_sum, ring_sup, out_sum, out_sup, out_mean);
  TD_LAUNCH_CHECK("stitch_live");
  return TDEED_OK;
}
