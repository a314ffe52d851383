// Event spotting on the resident score track: per-frame arg-max and high-recall statistics, then exact hard / soft
// non-maximum suppression per class (evalutil.nms_rounds is the written statement of the order) and an ordered compaction.
#include "common.h"

#define SPOT_MAX_CLASSES 64           // K1 - 1: the windows travel by value in the kernel arguments
#define SPOT_NT 1024                  // threads of a suppression / compaction workgroup
#define SPOT_LDS_FRAMES 16000         // longest track whose suppression state (9 bytes per frame) stays in LDS
#define SPOT_CB 8                     // flags a compaction thread loads at a time

struct SpotWindows {
  int w[SPOT_MAX_CLASSES];
};

// =========================================================================== frame events
// One thread per frame: pred = first maximum of the row (np.argmax), pred_score = that entry; pred_u8 (optional, K1 <= 256)
// the same index in one byte, the form in which it travels to the host.  Per class c >= 1 the frames
// with mean[f][c] >= hr (fp32 comparison): their number and the first of them, one integer atomic pair per wave and class
// (integer add / min: the result does not depend on the order).  first_frame arrives filled with L, count with 0.
__global__ __launch_bounds__(256) void frame_events_kernel(const float* __restrict__ mean, int L, int K1, float hr,
                                                           int* __restrict__ pred, unsigned char* __restrict__ pred_u8,
                                                           float* __restrict__ pred_score, int* __restrict__ first_frame, int* __restrict__ count) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  const bool in = f < L;
  const float* row = mean + (long)(in ? f : 0) * K1;
  const int wave_first = blockIdx.x * 256 + (threadIdx.x & ~63);
  float best = row[0];
  int bi = 0;
  for (int k = 1; k < K1; ++k) {
    const float x = row[k];
    if (x > best) { best = x; bi = k; }
    const unsigned long long m = __ballot(in && x >= hr);
    if (m != 0ull && (threadIdx.x & 63) == 0) {
      atomicAdd(count + k, __popcll(m));
      atomicMin(first_frame + k, wave_first + (__ffsll((long long)m) - 1));
    }
  }
  if (in) {
    pred[f] = bi;
    pred_score[f] = best;
    if (pred_u8) pred_u8[f] = (unsigned char)bi;
  }
}

extern "C" int tdeed_frame_events(const float* mean, int L, int K1, float hr_threshold, int* pred, unsigned char* pred_u8,
                                  float* pred_score,
                                  int* first_frame, int* count, void* stream) {
  TD_CHECK(mean && pred && pred_score && first_frame && count, "frame_events: null pointer");
  TD_CHECK(L > 0 && K1 > 1, "frame_events: bad sizes");
  TD_CHECK(!pred_u8 || K1 <= 256, "frame_events: %d columns do not fit the one-byte prediction", K1);
  hipLaunchKernelGGL(frame_events_kernel, dim3(cdiv(L, 256)), dim3(256), 0, (hipStream_t)stream, mean, L, K1, hr_threshold,
                     pred, pred_u8, pred_score, first_frame, count);
  TD_LAUNCH_CHECK("frame_events");
  return TDEED_OK;
}

// =========================================================================== suppression
// rank of class c among the classes that have a candidate, by (first candidate frame, class): the position of its label in
// the host's high-recall list (`_by_label`).  -1: no candidate.  K1 is small, every thread computes it from scalars.
__device__ __forceinline__ int spot_rank(const int* __restrict__ first_frame, int K1, int L, int c) {
  const int fc = first_frame[c];
  if (fc >= L) return -1;
  int r = 0;
  for (int o = 1; o < K1; ++o) {
    const int fo = first_frame[o];
    r += (fo < L && (fo < fc || (fo == fc && o < c))) ? 1 : 0;
  }
  return r;
}

// One workgroup per class (blockIdx.x + 1), dense over the frames: s[f] the candidate's current score (double), -inf for a
// frame that is no candidate or no longer live (the thresholds are > -inf), and win[f].  Thread t owns the frames t, t + NT,
// ...; it alone writes win[] of its frames.  A round:
//   A  every f with s[f] >= thr looks at the g within +-reach: beaten by an earlier g with s[g] >= s[f] or a later one with
//      s[g] > s[f].  No early exit: the loads of a window are independent, a wave takes as long as its slowest lane anyway;
//   -- barrier (also the vote "was anybody eligible": nobody -> done)
//   B  every winner p records its score, then hard: s[p-w..p+w] = -inf (two winners may both clear a frame: same value);
//      soft: s[g] = s[g] * (p-g)^2 / w^2 for g != p in p-w..p+w (-inf stays -inf), s[p] = -inf -- reach = 2w, so no g has
//      two winners;
//   -- barrier
// The best live candidate always wins, so at most `candidates` rounds: a bounded for loop.  IN_LDS: the two arrays live in
// LDS (L <= SPOT_LDS_FRAMES), otherwise in the caller's workspace (same CU, same L1: a workgroup barrier orders them).
template <bool IN_LDS>
__global__ __launch_bounds__(SPOT_NT) void nms_track_kernel(const float* __restrict__ mean, int L, int K1, float hr, double thr,
                                                            int soft, SpotWindows win_list, int is_list,
                                                            const int* __restrict__ first_frame, unsigned char* ws,
                                                            unsigned char* __restrict__ emitted, double* __restrict__ kept_score,
                                                            int* __restrict__ rounds_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char spot_smem[];
  const int c = blockIdx.x + 1;
  const int tid = threadIdx.x;
  unsigned char* em = emitted + (long)c * L;
  double* ks = kept_score + (long)c * L;
  const int rank = spot_rank(first_frame, K1, L, c);
  if (c == 1 && tid == 0) rounds_out[0] = 0;                   // the background column has no events
  if (rank < 0) {                                              // uniform: no candidate, nothing kept
    for (int f = tid; f < L; f += SPOT_NT) em[f] = 0;
    if (tid == 0) rounds_out[c] = 0;
    return;
  }
  TD_DEV_ASSERT(rank < K1 - 1);
  double* s;
  unsigned char* win;
  if (IN_LDS) {
    s = reinterpret_cast<double*>(spot_smem);
    win = spot_smem + (long)L * 8;
  } else {
    s = reinterpret_cast<double*>(ws) + (long)blockIdx.x * L;
    win = ws + (long)(K1 - 1) * L * 8 + (long)blockIdx.x * L;
  }
  const double dead = -__builtin_inf();
  const int w = is_list ? win_list.w[rank] : win_list.w[0];
  const double wsq = (double)w * (double)w;                    // float(w ** 2): exact below 2^53, one rounding above
  const int wr = w < L ? w : L;                                // no frame is further away than L - 1
  const int reach = soft ? 2 * wr : wr;
  int mine = 0;
  for (int f = tid; f < L; f += SPOT_NT) {
    const float x = mean[(long)f * K1 + c];
    const bool cand = x >= hr;
    s[f] = cand ? (double)x : dead;
    em[f] = 0;
    mine += cand ? 1 : 0;
  }
  // number of candidates = upper bound of the rounds; the second barrier also publishes s[]
  __shared__ int sh_cand;
  if (tid == 0) sh_cand = 0;
  __syncthreads();
  if (mine) atomicAdd(&sh_cand, mine);
  __syncthreads();
  const int max_rounds = sh_cand;
  int rounds = 0;
  for (int r = 0; r < max_rounds; ++r) {
    int any = 0;
    for (int f = tid; f < L; f += SPOT_NT) {
      const double sf = s[f];
      bool wn = sf >= thr;
      if (wn) {
        any = 1;
        const int lo = f - reach > 0 ? f - reach : 0;
        const int hi = f + reach < L - 1 ? f + reach : L - 1;
        TD_DEV_ASSERT(lo >= 0 && lo <= f && hi >= f && hi < L);
        bool beaten = false;
#pragma unroll 8
        for (int g = lo; g < f; ++g) beaten |= s[g] >= sf;     // an earlier frame wins ties
#pragma unroll 8
        for (int g = f + 1; g <= hi; ++g) beaten |= s[g] > sf;
        wn = !beaten;
      }
      win[f] = wn ? 1 : 0;
    }
    if (!__syncthreads_or(any)) break;
    ++rounds;
    for (int p = tid; p < L; p += SPOT_NT) {
      if (!win[p]) continue;
      em[p] = 1;
      ks[p] = s[p];
      const int lo = p - wr > 0 ? p - wr : 0;
      const int hi = p + wr < L - 1 ? p + wr : L - 1;
      TD_DEV_ASSERT(lo >= 0 && lo <= p && hi >= p && hi < L);
      if (soft) {
        for (int g = lo; g <= hi; ++g) {
          const long long d = (long long)(p - g);
          if (g != p) s[g] = s[g] * (double)(d * d) / wsq;     // the product first, then the quotient (no contraction possible)
        }
        s[p] = dead;
      } else {
        for (int g = lo; g <= hi; ++g) s[g] = dead;
      }
    }
    __syncthreads();
  }
  if (tid == 0) rounds_out[c] = rounds;
}

// =========================================================================== ordered compaction
// One workgroup: the kept events in the host's order -- ascending frame, within a frame by label appearance rank -- i.e. by
// the index i = f * nr + rank over the nr classes that have candidates.  Every thread owns a contiguous run of i: count,
// exclusive scan over the threads, write.  Deterministic: no atomics, the position depends on the flags alone.
__global__ __launch_bounds__(SPOT_NT) void spot_compact_kernel(const unsigned char* __restrict__ emitted,
                                                               const double* __restrict__ kept_score, int L, int K1,
                                                               const int* __restrict__ first_frame, int* __restrict__ out_frame,
                                                               int* __restrict__ out_class, unsigned char* __restrict__ out_class_u8,
                                                               double* __restrict__ out_score,
                                                               int* __restrict__ out_count) {
  __shared__ int order[SPOT_MAX_CLASSES];
  __shared__ int sh_nr;
  __shared__ int wave_tot[SPOT_NT / WAVE];
  const int tid = threadIdx.x;
  if (tid == 0) sh_nr = 0;
  __syncthreads();
  if (tid >= 1 && tid < K1) {
    const int r = spot_rank(first_frame, K1, L, tid);
    if (r >= 0) {
      TD_DEV_ASSERT(r < SPOT_MAX_CLASSES);
      order[r] = tid;
      atomicAdd(&sh_nr, 1);
    }
  }
  __syncthreads();
  const int nr = sh_nr;
  const long n = (long)L * nr;
  const long per = (n + SPOT_NT - 1) / SPOT_NT;
  const long i0 = per * tid < n ? per * tid : n;
  const long i1 = i0 + per < n ? i0 + per : n;
  int f0 = 0, r0 = 0;
  if (nr > 0) {
    f0 = (int)(i0 / nr);
    r0 = (int)(i0 - (long)f0 * nr);
  }
  // the flags of a run are loaded SPOT_CB at a time (independent loads in flight: one latency per batch, not per flag)
  int cnt = 0;
  {
    int f = f0, r = r0;
    for (long i = i0; i < i1; i += SPOT_CB) {
      unsigned char fl[SPOT_CB];
#pragma unroll
      for (int j = 0; j < SPOT_CB; ++j) {
        const bool in = i + j < i1;
        TD_DEV_ASSERT(!in || (f < L && r < nr));
        fl[j] = in ? emitted[(long)order[r] * L + f] : 0;
        if (in && ++r == nr) { r = 0; ++f; }
      }
#pragma unroll
      for (int j = 0; j < SPOT_CB; ++j) cnt += fl[j];
    }
  }
  // exclusive scan of cnt over the workgroup: inclusive scan inside each wave, then the totals of the waves before
  int inc = cnt;
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const int up = __shfl_up(inc, o, WAVE);
    if ((tid & 63) >= o) inc += up;
  }
  if ((tid & 63) == 63) wave_tot[tid >> 6] = inc;
  __syncthreads();
  int pos = inc - cnt;
  int total = 0;
#pragma unroll
  for (int v = 0; v < SPOT_NT / WAVE; ++v) {
    pos += v < (tid >> 6) ? wave_tot[v] : 0;
    total += wave_tot[v];
  }
  if (tid == 0) out_count[0] = total;
  {
    int f = f0, r = r0;
    for (long i = i0; i < i1; i += SPOT_CB) {
      unsigned char fl[SPOT_CB];
      int ff[SPOT_CB], cc[SPOT_CB];
#pragma unroll
      for (int j = 0; j < SPOT_CB; ++j) {
        const bool in = i + j < i1;
        ff[j] = f;
        cc[j] = in ? order[r] : 0;
        fl[j] = in ? emitted[(long)cc[j] * L + f] : 0;
        if (in && ++r == nr) { r = 0; ++f; }
      }
#pragma unroll
      for (int j = 0; j < SPOT_CB; ++j) {
        if (fl[j]) {
          TD_DEV_ASSERT(pos >= 0 && (long)pos < n);
          out_frame[pos] = ff[j];
          out_class[pos] = cc[j];
          if (out_class_u8) out_class_u8[pos] = (unsigned char)cc[j];     // K1 - 1 <= 64
          out_score[pos] = kept_score[(long)cc[j] * L + ff[j]];
          ++pos;
        }
      }
    }
  }
}

extern "C" long tdeed_nms_track_workspace(int L, int K1) {
  if (L <= SPOT_LDS_FRAMES || L <= 0 || K1 < 2) return 0;
  return (long)(K1 - 1) * L * 9;
}

extern "C" int tdeed_nms_track(const float* mean, int L, int K1, float hr_threshold, double threshold, int soft,
                               const int* windows, int n_windows, const int* first_frame, void* workspace,
                               unsigned char* emitted, double* kept_score, int* out_frame, int* out_class, unsigned char* out_class_u8,
                               double* out_score,
                               int* out_count, int* rounds, void* stream) {
  TD_CHECK(mean && windows && first_frame && emitted && kept_score && out_frame && out_class && out_score && out_count && rounds,
           "nms_track: null pointer");
  TD_CHECK(L > 0 && K1 > 1, "nms_track: bad sizes");
  TD_CHECK(L <= (1 << 29), "nms_track: L = %d, at most 2^29 frames", L);
  TD_CHECK(K1 - 1 <= SPOT_MAX_CLASSES, "nms_track: %d classes, at most %d", K1 - 1, SPOT_MAX_CLASSES);
  TD_CHECK((long)L * (K1 - 1) < (1l << 31), "nms_track: L * classes = %ld does not fit the int32 event count", (long)L * (K1 - 1));
  TD_CHECK(soft == 0 || soft == 1, "nms_track: soft must be 0 or 1");
  TD_CHECK(n_windows == 1 || n_windows >= K1 - 1, "nms_track: %d windows for %d classes (one, or one per class)", n_windows, K1 - 1);
  TD_CHECK(threshold == threshold && threshold > -__builtin_inf() && hr_threshold == hr_threshold && hr_threshold > -__builtin_inff(),
           "nms_track: thresholds must be numbers above -inf");
  SpotWindows wl = {};
  for (int i = 0; i < (n_windows == 1 ? 1 : K1 - 1); ++i) {
    TD_CHECK(windows[i] >= soft && windows[i] <= (1 << 30), "nms_track: window %d (soft suppression needs >= 1)", windows[i]);
    wl.w[i] = windows[i];
  }
  hipStream_t st = (hipStream_t)stream;
  const int is_list = n_windows == 1 ? 0 : 1;
  if (L <= SPOT_LDS_FRAMES) {
    static TdDevOnce once;
    if (!once.get()) {
      hipError_t e = hipFuncSetAttribute((const void*)nms_track_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         SPOT_LDS_FRAMES * 9);
      if (e != hipSuccess) { tdeed_set_error("nms_track: hipFuncSetAttribute: %s", hipGetErrorString(e)); return TDEED_ERR_RUNTIME; }
      once.set();
    }
    hipLaunchKernelGGL(nms_track_kernel<true>, dim3(K1 - 1), dim3(SPOT_NT), (size_t)L * 9, st, mean, L, K1, hr_threshold,
                       threshold, soft, wl, is_list, first_frame, (unsigned char*)nullptr, emitted, kept_score, rounds);
  } else {
    TD_CHECK(workspace && ((uintptr_t)workspace & 7) == 0, "nms_track: L = %d needs an 8-byte aligned workspace of %ld bytes", L,
             tdeed_nms_track_workspace(L, K1));
    hipLaunchKernelGGL(nms_track_kernel<false>, dim3(K1 - 1), dim3(SPOT_NT), 0, st, mean, L, K1, hr_threshold, threshold, soft, wl,
                       is_list, first_frame, (unsigned char*)workspace, emitted, kept_score, rounds);
  }
  TD_LAUNCH_CHECK("nms_track");
  hipLaunchKernelGGL(spot_compact_kernel, dim3(1), dim3(SPOT_NT), 0, st, emitted, kept_score, L, K1, first_frame, out_frame,
                     out_class, out_class_u8, out_score, out_count);
  TD_LAUNCH_CHECK("spot_compact");
  return TDEED_OK;
}
