// Training clips drawn from resident videos: strided clip windows gathered from the packed frame buffer, the mixup of two
// such windows without their uint8 intermediates, and the per-frame labels of a clip from its video's event list
// (dataset/frame.py:97-253 ActionSpotDataset._store_clips / _get_one / __getitem__; host twin: trainclips.py).
#include "common.h"

// =========================================================================== strided clip gather
// Packed frame that slot t of a clip reads, or -1 for a zero frame: the window is cut at the clip's OWN video (first /
// nframes are per clip), and a table entry that points outside the packed buffer is never followed.
__device__ __forceinline__ long train_clip_source(long total_frames, long first, long base, long nframes, int t, int stride) {
  const long f = base + (long)t * stride;
  const long p = first + f;
  return f >= 0 && f < nframes && first >= 0 && p < total_frames ? p : -1;
}

// PS (the ..._ps entries): the same bodies, but clip b samples every strides[b]-th frame (a DEVICE int32[B] table; a joint
// batch mixes clips of sets with different strides) -- one more 4-byte load per workgroup, nothing else differs.  An entry
// <= 0 is not followed: the clip's slots come out as zero frames, its label positions as 0 (the host refuses such a
// table before it is uploaded; the entry points cannot read it).
template <bool PS>
__device__ __forceinline__ int clip_stride(int stride, const int* __restrict__ strides, int b) {
  return PS ? strides[b] : stride;
}

// blockIdx.y = frame slot b*T + t (one 32-bit division per workgroup), 16-byte chunks as in clip_gather_v16_kernel
template <bool PS>
__global__ __launch_bounds__(256) void train_clip_gather_v16_kernel(const u32x4* __restrict__ frames, long total_frames,
                                                                    long chunks, const long* __restrict__ first,
                                                                    const long* __restrict__ base,
                                                                    const long* __restrict__ nframes, int T, int stride,
                                                                    const int* __restrict__ strides,
                                                                    u32x4* __restrict__ out) {
  const int slot = blockIdx.y;
  const int b = slot / T;
  const int s = clip_stride<PS>(stride, strides, b);
  const long p = !PS || s > 0 ? train_clip_source(total_frames, first[b], base[b], nframes[b], slot - b * T, s) : -1;
  const bool real = p >= 0;
  const u32x4* src = frames + (real ? p : 0) * chunks;
  u32x4* dst = out + (long)slot * chunks;
  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < chunks; i += (long)gridDim.x * 256)
    dst[i] = real ? src[i] : zero;
}

// frame sizes that are no multiple of 16 bytes (or unaligned buffers)
template <bool PS>
__global__ __launch_bounds__(256) void train_clip_gather_u8_kernel(const uint8_t* __restrict__ frames, long total_frames,
                                                                   long frame_bytes, const long* __restrict__ first,
                                                                   const long* __restrict__ base,
                                                                   const long* __restrict__ nframes, int T, int stride,
                                                                   const int* __restrict__ strides,
                                                                   uint8_t* __restrict__ out) {
  const int slot = blockIdx.y;
  const int b = slot / T;
  const int s = clip_stride<PS>(stride, strides, b);
  const long p = !PS || s > 0 ? train_clip_source(total_frames, first[b], base[b], nframes[b], slot - b * T, s) : -1;
  const bool real = p >= 0;
  const uint8_t* src = frames + (real ? p : 0) * frame_bytes;
  uint8_t* dst = out + (long)slot * frame_bytes;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < frame_bytes; i += (long)gridDim.x * 256)
    dst[i] = real ? src[i] : (uint8_t)0;
}

static int train_grid_x(long items) {
  const long g = cdiv(items, 256 * 4);                          // 4+ items per thread
  return (int)(g < 64 ? g : 64);
}

template <bool PS>
static int train_clip_gather_launch(const uint8_t* frames, long total_frames, long frame_bytes, const long* first,
                                    const long* base, const long* nframes, int B, int T, int stride, const int* strides,
                                    uint8_t* out, void* stream) {
  TD_CHECK(frames && first && base && nframes && out && (!PS || strides), "train_clip_gather: null pointer");
  TD_CHECK(total_frames > 0 && frame_bytes > 0 && B > 0 && T > 0, "train_clip_gather: bad sizes");
  TD_CHECK(PS || stride > 0, "train_clip_gather: stride must be positive");
  TD_CHECK((long)B * T <= 65535, "train_clip_gather: B*T=%ld frame slots exceed the grid's 65535", (long)B * T);
  hipStream_t st = (hipStream_t)stream;
  const bool v16 = frame_bytes % 16 == 0 && (((uintptr_t)frames | (uintptr_t)out) & 15) == 0;
  if (v16) {
    const long chunks = frame_bytes / 16;
    hipLaunchKernelGGL(train_clip_gather_v16_kernel<PS>, dim3(train_grid_x(chunks), B * T), dim3(256), 0, st,
                       (const u32x4*)frames, total_frames, chunks, first, base, nframes, T, stride, strides, (u32x4*)out);
  } else {
    hipLaunchKernelGGL(train_clip_gather_u8_kernel<PS>, dim3(train_grid_x(frame_bytes), B * T), dim3(256), 0, st, frames,
                       total_frames, frame_bytes, first, base, nframes, T, stride, strides, out);
  }
  TD_LAUNCH_CHECK("train_clip_gather");
  return TDEED_OK;
}

extern "C" int tdeed_train_clip_gather_u8(const uint8_t* frames, long total_frames, long frame_bytes, const long* first,
                                          const long* base, const long* nframes, int B, int T, int stride, uint8_t* out,
                                          void* stream) {
  return train_clip_gather_launch<false>(frames, total_frames, frame_bytes, first, base, nframes, B, T, stride, nullptr, out,
                                         stream);
}

extern "C" int tdeed_train_clip_gather_u8_ps(const uint8_t* frames, long total_frames, long frame_bytes, const long* first,
                                             const long* base, const long* nframes, int B, int T, const int* strides,
                                             uint8_t* out, void* stream) {
  return train_clip_gather_launch<true>(frames, total_frames, frame_bytes, first, base, nframes, B, T, 0, strides, out, stream);
}

// =========================================================================== gather + mixup
// out[b][t] = lam[b] * A[b][t] + (1 - lam[b]) * B[b][t] with A / B the two gathered windows (a zero frame where padded):
// the expression of mix_frames_kernel (trunk_bwd.hip) in the contraction the compiler gives it there, fma(l, a, (1 - l) * b),
// spelled out: left to -ffp-contract the byte path below came out as two products and an add, with other bits.  The result
// carries the bits tdeed_mix_frames gives on the two gathered uint8 batches, which are never written.
__device__ __forceinline__ float mix_one(float l, float a, float b) { return __builtin_fmaf(l, a, (1.f - l) * b); }

template <bool PS>
__global__ __launch_bounds__(256) void train_clip_gather_mix_v4_kernel(
    const uint8_t* __restrict__ frames, long total_frames, long frame_bytes, const long* __restrict__ first_a,
    const long* __restrict__ base_a, const long* __restrict__ nframes_a, const long* __restrict__ first_b,
    const long* __restrict__ base_b, const long* __restrict__ nframes_b, const float* __restrict__ lam, int T, int stride,
    const int* __restrict__ strides, float* __restrict__ out) {
  const int slot = blockIdx.y;
  const int b = slot / T, t = slot - b * T;
  const int s = clip_stride<PS>(stride, strides, b);
  const bool ok = !PS || s > 0;
  const long pa = ok ? train_clip_source(total_frames, first_a[b], base_a[b], nframes_a[b], t, s) : -1;
  const long pb = ok ? train_clip_source(total_frames, first_b[b], base_b[b], nframes_b[b], t, s) : -1;
  const float l = lam[b];
  const uint8_t* sa = frames + (pa >= 0 ? pa : 0) * frame_bytes;
  const uint8_t* sb = frames + (pb >= 0 ? pb : 0) * frame_bytes;
  float* dst = out + (long)slot * frame_bytes;
  const uchar4 zero = {0, 0, 0, 0};
  const long quads = frame_bytes / 4;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < quads; q += (long)gridDim.x * 256) {
    const uchar4 va = pa >= 0 ? *reinterpret_cast<const uchar4*>(sa + q * 4) : zero;
    const uchar4 vb = pb >= 0 ? *reinterpret_cast<const uchar4*>(sb + q * 4) : zero;
    f32x4 o = {mix_one(l, (float)va.x, (float)vb.x), mix_one(l, (float)va.y, (float)vb.y),
               mix_one(l, (float)va.z, (float)vb.z), mix_one(l, (float)va.w, (float)vb.w)};
    *reinterpret_cast<f32x4*>(dst + q * 4) = o;
  }
}

// frame sizes that are no multiple of 4 bytes (or unaligned buffers)
template <bool PS>
__global__ __launch_bounds__(256) void train_clip_gather_mix_u8_kernel(
    const uint8_t* __restrict__ frames, long total_frames, long frame_bytes, const long* __restrict__ first_a,
    const long* __restrict__ base_a, const long* __restrict__ nframes_a, const long* __restrict__ first_b,
    const long* __restrict__ base_b, const long* __restrict__ nframes_b, const float* __restrict__ lam, int T, int stride,
    const int* __restrict__ strides, float* __restrict__ out) {
  const int slot = blockIdx.y;
  const int b = slot / T, t = slot - b * T;
  const int s = clip_stride<PS>(stride, strides, b);
  const bool ok = !PS || s > 0;
  const long pa = ok ? train_clip_source(total_frames, first_a[b], base_a[b], nframes_a[b], t, s) : -1;
  const long pb = ok ? train_clip_source(total_frames, first_b[b], base_b[b], nframes_b[b], t, s) : -1;
  const float l = lam[b];
  const uint8_t* sa = frames + (pa >= 0 ? pa : 0) * frame_bytes;
  const uint8_t* sb = frames + (pb >= 0 ? pb : 0) * frame_bytes;
  float* dst = out + (long)slot * frame_bytes;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < frame_bytes; i += (long)gridDim.x * 256) {
    const uint8_t a = pa >= 0 ? sa[i] : (uint8_t)0, c = pb >= 0 ? sb[i] : (uint8_t)0;
    dst[i] = mix_one(l, (float)a, (float)c);
  }
}

template <bool PS>
static int train_clip_gather_mix_launch(const uint8_t* frames, long total_frames, long frame_bytes, const long* first_a,
                                        const long* base_a, const long* nframes_a, const long* first_b, const long* base_b,
                                        const long* nframes_b, const float* lam, int B, int T, int stride, const int* strides,
                                        float* out, void* stream) {
  TD_CHECK(frames && first_a && base_a && nframes_a && first_b && base_b && nframes_b && lam && out && (!PS || strides),
           "train_clip_gather_mix: null pointer");
  TD_CHECK(total_frames > 0 && frame_bytes > 0 && B > 0 && T > 0, "train_clip_gather_mix: bad sizes");
  TD_CHECK(PS || stride > 0, "train_clip_gather_mix: stride must be positive");
  TD_CHECK((long)B * T <= 65535, "train_clip_gather_mix: B*T=%ld frame slots exceed the grid's 65535", (long)B * T);
  TD_CHECK(((uintptr_t)out & 3) == 0, "train_clip_gather_mix: out is not aligned for fp32");
  hipStream_t st = (hipStream_t)stream;
  const bool v4 = frame_bytes % 4 == 0 && ((uintptr_t)frames & 3) == 0 && ((uintptr_t)out & 15) == 0;
  if (v4) {
    hipLaunchKernelGGL(train_clip_gather_mix_v4_kernel<PS>, dim3(train_grid_x(frame_bytes / 4), B * T), dim3(256), 0, st,
                       frames, total_frames, frame_bytes, first_a, base_a, nframes_a, first_b, base_b, nframes_b, lam, T, stride,
                       strides, out);
  } else {
    hipLaunchKernelGGL(train_clip_gather_mix_u8_kernel<PS>, dim3(train_grid_x(frame_bytes), B * T), dim3(256), 0, st, frames,
                       total_frames, frame_bytes, first_a, base_a, nframes_a, first_b, base_b, nframes_b, lam, T, stride,
                       strides, out);
  }
  TD_LAUNCH_CHECK("train_clip_gather_mix");
  return TDEED_OK;
}

extern "C" int tdeed_train_clip_gather_mix_f32(const uint8_t* frames, long total_frames, long frame_bytes,
                                               const long* first_a, const long* base_a, const long* nframes_a,
                                               const long* first_b, const long* base_b, const long* nframes_b,
                                               const float* lam, int B, int T, int stride, float* out, void* stream) {
  return train_clip_gather_mix_launch<false>(frames, total_frames, frame_bytes, first_a, base_a, nframes_a, first_b, base_b,
                                             nframes_b, lam, B, T, stride, nullptr, out, stream);
}

extern "C" int tdeed_train_clip_gather_mix_f32_ps(const uint8_t* frames, long total_frames, long frame_bytes,
                                                  const long* first_a, const long* base_a, const long* nframes_a,
                                                  const long* first_b, const long* base_b, const long* nframes_b,
                                                  const float* lam, int B, int T, const int* strides, float* out,
                                                  void* stream) {
  return train_clip_gather_mix_launch<true>(frames, total_frames, frame_bytes, first_a, base_a, nframes_a, first_b, base_b,
                                            nframes_b, lam, B, T, 0, strides, out, stream);
}

// =========================================================================== clip labels
// One thread per (clip, t).  It walks the events of the clip's video in list order; event e sits at clip position
// idx = floor((ev_frame[e] - base) / stride) and labels the positions within r of it (dataset/frame.py:151-159).  The
// reference writes the events one after the other into the label row, so the LAST event in list order that reaches t
// wins: the thread keeps it.  No atomics.  Python's // floors; C's / truncates towards zero, hence floor_div.
__device__ __forceinline__ long floor_div(long a, long b) {      // b > 0
  const long q = a / b;
  return a - q * b < 0 ? q - 1 : q;
}

template <bool PS>
__global__ __launch_bounds__(256) void clip_labels_kernel(const long* __restrict__ clip_video, const long* __restrict__ clip_base,
                                                          int n, int T, int stride, const int* __restrict__ strides, int r,
                                                          const int* __restrict__ ev_off,
                                                          const int* __restrict__ ev_frame, const int* __restrict__ ev_class,
                                                          int nv, int n_events, long* __restrict__ label,
                                                          long* __restrict__ labelD) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)n * T) return;
  const int c = (int)(i / T);
  const long t = i - (long)c * T;
  const long v = clip_video[c];
  const int s = clip_stride<PS>(stride, strides, c);
  long lab = 0, dis = 0;
  if (v >= 0 && v < nv && (!PS || s > 0)) {                      // a table entry outside the event lists reads nothing
    const long base = clip_base[c];
    int e0 = ev_off[v], e1 = ev_off[v + 1];
    e0 = e0 > 0 ? e0 : 0;
    e1 = e1 < n_events ? e1 : n_events;
    for (int e = e0; e < e1; ++e) {
      const long d = t - floor_div((long)ev_frame[e] - base, s);
      if (d >= -r && d <= r) {
        lab = ev_class[e];
        dis = d;
      }
    }
  }
  label[i] = lab;
  if (labelD) labelD[i] = dis;
}

template <bool PS>
static int clip_labels_launch(const long* clip_video, const long* clip_base, int n, int T, int stride, const int* strides, int r,
                              const int* ev_off, const int* ev_frame, const int* ev_class, int nv, int n_events, long* label,
                              long* labelD, void* stream) {
  TD_CHECK(clip_video && clip_base && ev_off && label && (!PS || strides), "clip_labels: null pointer");
  TD_CHECK(n_events == 0 || (ev_frame && ev_class), "clip_labels: null event arrays");
  TD_CHECK(n > 0 && T > 0 && nv > 0 && n_events >= 0, "clip_labels: bad sizes");
  TD_CHECK(PS || stride > 0, "clip_labels: stride must be positive");
  TD_CHECK(r >= 0, "clip_labels: the radius must not be negative");
  const long total = (long)n * T;
  TD_CHECK(total <= 0x7fffffffL, "clip_labels: n*T=%ld label positions exceed 2^31 - 1", total);
  hipLaunchKernelGGL(clip_labels_kernel<PS>, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, clip_video,
                     clip_base, n, T, stride, strides, r, ev_off, ev_frame, ev_class, nv, n_events, label, labelD);
  TD_LAUNCH_CHECK("clip_labels");
  return TDEED_OK;
}

extern "C" int tdeed_clip_labels(const long* clip_video, const long* clip_base, int n, int T, int stride, int r,
                                 const int* ev_off, const int* ev_frame, const int* ev_class, int nv, int n_events,
                                 long* label, long* labelD, void* stream) {
  return clip_labels_launch<false>(clip_video, clip_base, n, T, stride, nullptr, r, ev_off, ev_frame, ev_class, nv, n_events,
                                   label, labelD, stream);
}

extern "C" int tdeed_clip_labels_ps(const long* clip_video, const long* clip_base, int n, int T, const int* strides, int r,
                                    const int* ev_off, const int* ev_frame, const int* ev_class, int nv, int n_events,
                                    long* label, long* labelD, void* stream) {
  return clip_labels_launch<true>(clip_video, clip_base, n, T, 0, strides, r, ev_off, ev_frame, ev_class, nv, n_events, label,
                                  labelD, stream);
}
