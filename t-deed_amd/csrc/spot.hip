// Event spotting on the resident score track: per-frame arg-max and high-recall statistics, then exact hard / soft
// non-maximum suppression per class (evalutil.nms_rounds is the written statement of the order) and an ordered compaction.
#include "common.h"

#define SPOT_MAX_CLASSES 64           // K1 - 1: the windows travel by value in the kernel arguments
#define SPOT_NT 1024                  // threads of the largest suppression / compaction workgroup (tdeed_nms_track_seg_threads)
#define SPOT_LDS_FRAMES 16000         // longest track whose suppression state (9 bytes per frame) stays in LDS
#define SPOT_CB 8                     // flags a compaction thread loads at a time

struct SpotWindows {
  int w[SPOT_MAX_CLASSES];
};

// =========================================================================== frame events
// One thread per frame of a track that packs nv videos one after the other (one video: nv = 1): pred = first maximum of the
// row (np.argmax), pred_score = that entry; pred_u8 (optional, K1 <= 256) the same index in one byte, the form in which it
// travels to the host.  Per video and class c >= 1 the frames with mean[f][c] >= hr (fp32 comparison): their number and the
// first of them, one integer atomic pair per wave and class (integer add / min: the result does not depend on the order).
// blockIdx.y = video, blockIdx.x = block of 256 frames inside it, so no wave straddles two videos (workgroups past the end
// of a short video leave at once).  Frames are video-local in first_frame [nv][K1] (arrives filled with the video's length),
// count [nv][K1] (arrives 0).
__global__ __launch_bounds__(256) void frame_events_seg_kernel(const float* __restrict__ mean, const int* __restrict__ seg_off,
                                                               int L_total, int K1, float hr, int* __restrict__ pred,
                                                               unsigned char* __restrict__ pred_u8, float* __restrict__ pred_score,
                                                               int* __restrict__ first_frame, int* __restrict__ count) {
  const int v = blockIdx.y;
  const int p0 = seg_off[v];
  const int L = seg_off[v + 1] - p0;
  if (p0 < 0 || L <= 0 || (long)p0 + L > L_total || (int)blockIdx.x * 256 >= L) return;      // uniform
  const int f = blockIdx.x * 256 + threadIdx.x;
  const bool in = f < L;
  const float* row = mean + (long)(p0 + (in ? f : 0)) * K1;
  const int wave_first = blockIdx.x * 256 + (threadIdx.x & ~63);
  int* ff = first_frame + (long)v * K1;
  int* cn = count + (long)v * K1;
  float best = row[0];
  int bi = 0;
  for (int k = 1; k < K1; ++k) {
    const float x = row[k];
    if (x > best) { best = x; bi = k; }
    const unsigned long long m = __ballot(in && x >= hr);
    if (m != 0ull && (threadIdx.x & 63) == 0) {
      atomicAdd(cn + k, __popcll(m));
      atomicMin(ff + k, wave_first + (__ffsll((long long)m) - 1));
    }
  }
  if (in) {
    pred[p0 + f] = bi;
    pred_score[p0 + f] = best;
    if (pred_u8) pred_u8[p0 + f] = (unsigned char)bi;
  }
}

extern "C" int tdeed_frame_events_seg(const float* mean, const int* seg_off, int nv, int L_total, int max_len, int K1,
                                      float hr_threshold, int* pred, unsigned char* pred_u8, float* pred_score, int* first_frame,
                                      int* count, void* stream) {
  TD_CHECK(mean && seg_off && pred && pred_score && first_frame && count, "frame_events_seg: null pointer");
  TD_CHECK(L_total > 0 && K1 > 1 && nv > 0 && max_len > 0 && max_len <= L_total, "frame_events_seg: bad sizes");
  TD_CHECK(nv <= 65535, "frame_events_seg: %d videos in one group, at most 65535", nv);
  TD_CHECK(!pred_u8 || K1 <= 256, "frame_events_seg: %d columns do not fit the one-byte prediction", K1);
  hipLaunchKernelGGL(frame_events_seg_kernel, dim3(cdiv(max_len, 256), nv), dim3(256), 0, (hipStream_t)stream, mean, seg_off,
                     L_total, K1, hr_threshold, pred, pred_u8, pred_score, first_frame, count);
  TD_LAUNCH_CHECK("frame_events_seg");
  return TDEED_OK;
}

// =========================================================================== frame error and foreground-F1 counters
// The label-dependent counters of evalutil.frame_events(labels=...) (util/eval.py:34-84) over the packed track of a group:
// per frame pred = frame_events_seg_kernel's arg-max (first maximum), true = the packed uint8 label.  stats int64
// [2 + 3*K1] is added to: [0] frames, [1] frames with pred != true, then (tp, fp, fn) at 2 + 3*k for k = 0 ("any": foreground
// against background) and every class k >= 1:
//   any      tp: pred != 0 and true != 0    fp: pred != 0 and true == 0    fn: pred == 0 and true != 0
//   class k  tp: pred == true == k          fp: pred == k != true          fn: true == k != pred
// Integers, so any order of accumulation gives the same sums: int32 partials of a workgroup in LDS (the five frame-level
// counters from wave ballots, at most two class counters per frame by LDS atomics), then one 64-bit vector atomic add per
// counter the workgroup touched.  The grid is bounded (FS_MAX_BLOCKS workgroups stride over the frames), so a pass issues at
// most FS_MAX_BLOCKS * (2 + 3*K1) global atomics whatever the length of the track.
#define FS_NT 256
#define FS_MAX_BLOCKS 256
#define FS_MAX_COUNTERS (2 + 3 * 256)

__global__ __launch_bounds__(FS_NT) void frame_stats_seg_kernel(const float* __restrict__ mean, const unsigned char* __restrict__ labels,
                                                              int L_total, int K1, unsigned long long* __restrict__ stats) {
  __shared__ int part[FS_MAX_COUNTERS];
  const int nc = 2 + 3 * K1;
  for (int j = threadIdx.x; j < nc; j += FS_NT) part[j] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  // every wave runs the same number of rounds (the ballots need whole waves): frames past the end are masked out
  for (long base = (long)blockIdx.x * FS_NT; base < L_total; base += (long)gridDim.x * FS_NT) {
    const long f = base + threadIdx.x;
    const bool in = f < L_total;
    const float* row = mean + (in ? f : 0) * K1;
    float best = row[0];
    int p = 0;
    for (int k = 1; k < K1; ++k) {
      const float x = row[k];
      if (x > best) { best = x; p = k; }
    }
    const int t = in ? (int)labels[f] : 0;
    const bool ok = in && t < K1;                                      // a label outside the columns is not followed
    const unsigned long long m_in = __ballot(ok);
    const unsigned long long m_err = __ballot(ok && p != t);
    const unsigned long long m_tp = __ballot(ok && p != 0 && t != 0);
    const unsigned long long m_fp = __ballot(ok && p != 0 && t == 0);
    const unsigned long long m_fn = __ballot(ok && p == 0 && t != 0);
    if (lane == 0) {
      if (m_in) atomicAdd(&part[0], __popcll(m_in));
      if (m_err) atomicAdd(&part[1], __popcll(m_err));
      if (m_tp) atomicAdd(&part[2], __popcll(m_tp));
      if (m_fp) atomicAdd(&part[3], __popcll(m_fp));
      if (m_fn) atomicAdd(&part[4], __popcll(m_fn));
    }
    if (ok) {
      if (p == t) {
        if (p != 0) atomicAdd(&part[2 + 3 * p], 1);
      } else {
        if (p != 0) atomicAdd(&part[2 + 3 * p + 1], 1);
        if (t != 0) atomicAdd(&part[2 + 3 * t + 2], 1);
      }
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < nc; j += FS_NT) {
    const int x = part[j];
    if (x != 0) atomicAdd(stats + j, (unsigned long long)x);
  }
}

extern "C" int tdeed_frame_stats_seg(const float* mean, const unsigned char* labels, int L_total, int K1, long* stats, void* stream) {
  TD_CHECK(mean && labels && stats, "frame_stats_seg: null pointer");
  TD_CHECK(L_total > 0 && K1 > 1 && K1 <= 256, "frame_stats_seg: %d frames, %d columns (2 to 256: the labels are bytes)", L_total, K1);
  const int blocks = cdiv(L_total, FS_NT) < FS_MAX_BLOCKS ? cdiv(L_total, FS_NT) : FS_MAX_BLOCKS;
  hipLaunchKernelGGL(frame_stats_seg_kernel, dim3(blocks), dim3(FS_NT), 0, (hipStream_t)stream, mean, labels, L_total, K1,
                     reinterpret_cast<unsigned long long*>(stats));
  TD_LAUNCH_CHECK("frame_stats_seg");
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
// The work of one workgroup of NT threads on class c of one track of L frames: mean / em / ks point at the track's first frame
// (rows of K1 floats; flags and scores of class c), s / win at its state, first_frame / rounds_out at its K1 entries.
template <int NT>
__device__ __forceinline__ void nms_track_body(const float* __restrict__ mean, int L, int K1, int c, float hr, double thr, int soft,
                                               const SpotWindows& win_list, int is_list, const int* __restrict__ first_frame,
                                               double* s, unsigned char* win, unsigned char* __restrict__ em,
                                               double* __restrict__ ks, int* __restrict__ rounds_out) {
  const int tid = threadIdx.x;
  const int rank = spot_rank(first_frame, K1, L, c);
  if (c == 1 && tid == 0) rounds_out[0] = 0;                   // the background column has no events
  if (rank < 0) {                                              // uniform: no candidate, nothing kept
    for (int f = tid; f < L; f += NT) em[f] = 0;
    if (tid == 0) rounds_out[c] = 0;
    return;
  }
  TD_DEV_ASSERT(rank < K1 - 1);
  const double dead = -__builtin_inf();
  const int w = is_list ? win_list.w[rank] : win_list.w[0];
  const double wsq = (double)w * (double)w;                    // float(w ** 2): exact below 2^53, one rounding above
  const int wr = w < L ? w : L;                                // no frame is further away than L - 1
  const int reach = soft ? 2 * wr : wr;
  int mine = 0;
  for (int f = tid; f < L; f += NT) {
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
    for (int f = tid; f < L; f += NT) {
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
    for (int p = tid; p < L; p += NT) {
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

// blockIdx.x + 1 = class, blockIdx.y = video of the packed track.  The workgroup runs the body above on
// its video's segment of the packed track with that video's first_frame row (video-local frames, windows and rank);
// emitted / kept_score are [K1][L_total], the state in LDS is sized by the group's longest video, the workspace form keeps
// [K1-1][L_total] doubles and as many bytes.  NT threads: chosen by the launcher from the longest video.
template <bool IN_LDS, int NT>
__global__ __launch_bounds__(NT) void nms_track_seg_kernel(const float* __restrict__ mean, const int* __restrict__ seg_off,
                                                           int L_total, int max_len, int K1, float hr, double thr, int soft,
                                                           SpotWindows win_list, int is_list, const int* __restrict__ first_frame,
                                                           unsigned char* ws, unsigned char* __restrict__ emitted,
                                                           double* __restrict__ kept_score, int* __restrict__ rounds_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char spot_smem[];
  const int c = blockIdx.x + 1;
  const int v = blockIdx.y;
  const int p0 = seg_off[v];
  const int L = seg_off[v + 1] - p0;
  if (p0 < 0 || L <= 0 || L > max_len || (long)p0 + L > L_total) return;      // uniform: a table that does not fit the buffers
  double* s;
  unsigned char* win;
  if (IN_LDS) {
    s = reinterpret_cast<double*>(spot_smem);
    win = spot_smem + (long)L * 8;
  } else {
    s = reinterpret_cast<double*>(ws) + (long)blockIdx.x * L_total + p0;
    win = ws + (long)(K1 - 1) * L_total * 8 + (long)blockIdx.x * L_total + p0;
  }
  nms_track_body<NT>(mean + (long)p0 * K1, L, K1, c, hr, thr, soft, win_list, is_list, first_frame + (long)v * K1, s, win,
                     emitted + (long)c * L_total + p0, kept_score + (long)c * L_total + p0, rounds_out + (long)v * K1);
}

// =========================================================================== ordered compaction
// One workgroup: the kept events in the host's order -- ascending frame, within a frame by label appearance rank -- i.e. by
// the index i = f * nr + rank over the nr classes that have candidates.  Every thread owns a contiguous run of i: count,
// exclusive scan over the threads, write.  Deterministic: no atomics, the position depends on the flags alone.
// emitted / kept_score: [K1][stride] with this track's L frames at the front of every row; NT threads.
template <int NT>
__device__ __forceinline__ void spot_compact_body(const unsigned char* __restrict__ emitted, const double* __restrict__ kept_score,
                                                  long stride, int L, int K1, const int* __restrict__ first_frame,
                                                  int* __restrict__ out_frame, int* __restrict__ out_class,
                                                  unsigned char* __restrict__ out_class_u8, double* __restrict__ out_score,
                                                  int* __restrict__ out_count) {
  __shared__ int order[SPOT_MAX_CLASSES];
  __shared__ int sh_nr;
  __shared__ int wave_tot[NT / WAVE];
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
  const long per = (n + NT - 1) / NT;
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
        fl[j] = in ? emitted[(long)order[r] * stride + f] : 0;
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
  for (int v = 0; v < NT / WAVE; ++v) {
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
        fl[j] = in ? emitted[(long)cc[j] * stride + f] : 0;
        if (in && ++r == nr) { r = 0; ++f; }
      }
#pragma unroll
      for (int j = 0; j < SPOT_CB; ++j) {
        if (fl[j]) {
          TD_DEV_ASSERT(pos >= 0 && (long)pos < n);
          out_frame[pos] = ff[j];
          if (out_class) out_class[pos] = cc[j];
          if (out_class_u8) out_class_u8[pos] = (unsigned char)cc[j];     // K1 - 1 <= 64
          out_score[pos] = kept_score[(long)cc[j] * stride + ff[j]];
          ++pos;
        }
      }
    }
  }
}

// The videos of a packed track, three steps.  (1) One workgroup per video compacts its own list, in the order
// above, into the video's share of a staging list (room for L_v * (K1-1) events from seg_off[v] * (K1-1) on) and writes its
// length.  (2) One workgroup turns the nv lengths into event_off[nv+1] (exclusive scan, every thread a contiguous run of
// videos).  (3) One workgroup per video moves its staged list to event_off[v] of the dense list: the videos' lists follow each
// other in video order and the host copies one contiguous range.  Positions depend on the flags alone: no atomics.
template <int NT>
__global__ __launch_bounds__(NT) void spot_compact_seg_kernel(const unsigned char* __restrict__ emitted,
                                                              const double* __restrict__ kept_score,
                                                              const int* __restrict__ seg_off, int L_total, int max_len, int K1,
                                                              const int* __restrict__ first_frame, int* __restrict__ st_frame,
                                                              unsigned char* __restrict__ st_class_u8, double* __restrict__ st_score,
                                                              int* __restrict__ st_count) {
  const int v = blockIdx.x;
  const int p0 = seg_off[v];
  const int L = seg_off[v + 1] - p0;
  if (p0 < 0 || L <= 0 || L > max_len || (long)p0 + L > L_total) {            // uniform: a table that does not fit the buffers
    if (threadIdx.x == 0) st_count[v] = 0;
    return;
  }
  const long o = (long)p0 * (K1 - 1);
  spot_compact_body<NT>(emitted + p0, kept_score + p0, L_total, L, K1, first_frame + (long)v * K1, st_frame + o, nullptr,
                        st_class_u8 + o, st_score + o, st_count + v);
}

__global__ __launch_bounds__(SPOT_NT) void spot_event_offsets_kernel(const int* __restrict__ st_count, int nv,
                                                                     int* __restrict__ event_off) {
  __shared__ int wave_tot[SPOT_NT / WAVE];
  const int tid = threadIdx.x;
  const int per = (nv + SPOT_NT - 1) / SPOT_NT;
  const int v0 = per * tid < nv ? per * tid : nv;
  const int v1 = v0 + per < nv ? v0 + per : nv;
  int cnt = 0;
  for (int v = v0; v < v1; ++v) cnt += st_count[v];
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
  for (int w = 0; w < SPOT_NT / WAVE; ++w) {
    pos += w < (tid >> 6) ? wave_tot[w] : 0;
    total += wave_tot[w];
  }
  for (int v = v0; v < v1; ++v) {
    event_off[v] = pos;
    pos += st_count[v];
  }
  if (tid == 0) event_off[nv] = total;
}

__global__ __launch_bounds__(256) void spot_pack_events_kernel(const int* __restrict__ seg_off, int L_total, int K1,
                                                               const int* __restrict__ event_off,
                                                               const int* __restrict__ st_frame,
                                                               const unsigned char* __restrict__ st_class_u8,
                                                               const double* __restrict__ st_score, int* __restrict__ out_frame,
                                                               unsigned char* __restrict__ out_class_u8,
                                                               double* __restrict__ out_score) {
  const int v = blockIdx.x;
  const int p0 = seg_off[v];
  const int e0 = event_off[v];
  const int m = event_off[v + 1] - e0;
  const long cap = (long)L_total * (K1 - 1);
  const long o = (long)p0 * (K1 - 1);
  if (p0 < 0 || m <= 0 || o + m > cap || e0 < 0 || (long)e0 + m > cap) return;      // uniform
  for (int i = threadIdx.x; i < m; i += 256) {
    out_frame[e0 + i] = st_frame[o + i];
    out_class_u8[e0 + i] = st_class_u8[o + i];
    out_score[e0 + i] = st_score[o + i];
  }
}

extern "C" long tdeed_nms_track_seg_workspace(int L_total, int max_len, int K1) {
  if (max_len <= SPOT_LDS_FRAMES || L_total <= 0 || max_len <= 0 || K1 < 2) return 0;
  return (long)(K1 - 1) * L_total * 9;
}

namespace {
struct SpotSegArgs {
  const float* mean; const int* seg_off; int nv, L_total, max_len, K1; float hr; double thr; int soft; SpotWindows wl; int is_list;
  const int* first_frame; unsigned char* ws; unsigned char* emitted; double* kept_score; int* st_frame; unsigned char* st_class_u8;
  double* st_score; int* st_count; int* rounds; hipStream_t st;
};

// suppression + per-video compaction with workgroups of NT threads
template <int NT>
int spot_seg_launch(const SpotSegArgs& a) {
  if (a.max_len <= SPOT_LDS_FRAMES) {
    const size_t lds = (size_t)a.max_len * 9;
    if (lds > 32768) {                                           // beyond what a launch may ask for without the attribute
      static TdDevOnce once;
      if (!once.get()) {
        hipError_t e = hipFuncSetAttribute((const void*)nms_track_seg_kernel<true, NT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           SPOT_LDS_FRAMES * 9);
        if (e != hipSuccess) { tdeed_set_error("nms_track_seg: hipFuncSetAttribute: %s", hipGetErrorString(e)); return TDEED_ERR_RUNTIME; }
        once.set();
      }
    }
    hipLaunchKernelGGL((nms_track_seg_kernel<true, NT>), dim3(a.K1 - 1, a.nv), dim3(NT), lds, a.st, a.mean, a.seg_off, a.L_total,
                       a.max_len, a.K1, a.hr, a.thr, a.soft, a.wl, a.is_list, a.first_frame, (unsigned char*)nullptr, a.emitted,
                       a.kept_score, a.rounds);
  } else {
    hipLaunchKernelGGL((nms_track_seg_kernel<false, NT>), dim3(a.K1 - 1, a.nv), dim3(NT), 0, a.st, a.mean, a.seg_off, a.L_total,
                       a.max_len, a.K1, a.hr, a.thr, a.soft, a.wl, a.is_list, a.first_frame, a.ws, a.emitted, a.kept_score, a.rounds);
  }
  TD_LAUNCH_CHECK("nms_track_seg");
  hipLaunchKernelGGL(spot_compact_seg_kernel<NT>, dim3(a.nv), dim3(NT), 0, a.st, a.emitted, a.kept_score, a.seg_off, a.L_total,
                     a.max_len, a.K1, a.first_frame, a.st_frame, a.st_class_u8, a.st_score, a.st_count);
  TD_LAUNCH_CHECK("spot_compact_seg");
  return TDEED_OK;
}
}  // namespace

// threads of a suppression / compaction workgroup for a group whose longest video has max_len frames: one frame per thread up
// to 1024 (a thread owns the frames t, t + NT, ...)
extern "C" int tdeed_nms_track_seg_threads(int max_len) {
  return max_len <= 128 ? 128 : max_len <= 256 ? 256 : max_len <= 512 ? 512 : SPOT_NT;
}

extern "C" int tdeed_nms_track_seg(const float* mean, const int* seg_off, int nv, int L_total, int max_len, int K1,
                                   float hr_threshold, double threshold, int soft, const int* windows, int n_windows,
                                   const int* first_frame, void* workspace, unsigned char* emitted, double* kept_score,
                                   int* st_frame, unsigned char* st_class_u8, double* st_score, int* st_count, int* out_frame,
                                   unsigned char* out_class_u8, double* out_score, int* event_off, int* rounds, void* stream) {
  TD_CHECK(mean && seg_off && windows && first_frame && emitted && kept_score && st_frame && st_class_u8 && st_score && st_count &&
               out_frame && out_class_u8 && out_score && event_off && rounds,
           "nms_track_seg: null pointer");
  TD_CHECK(L_total > 0 && K1 > 1 && nv > 0 && max_len > 0 && max_len <= L_total, "nms_track_seg: bad sizes");
  TD_CHECK(nv <= 65535, "nms_track_seg: %d videos in one group, at most 65535", nv);
  TD_CHECK(L_total <= (1 << 29), "nms_track_seg: %d frames, at most 2^29", L_total);
  TD_CHECK(K1 - 1 <= SPOT_MAX_CLASSES, "nms_track_seg: %d classes, at most %d", K1 - 1, SPOT_MAX_CLASSES);
  TD_CHECK((long)L_total * (K1 - 1) < (1l << 31), "nms_track_seg: frames * classes = %ld does not fit the int32 event count",
           (long)L_total * (K1 - 1));
  TD_CHECK(soft == 0 || soft == 1, "nms_track_seg: soft must be 0 or 1");
  TD_CHECK(n_windows == 1 || n_windows >= K1 - 1, "nms_track_seg: %d windows for %d classes (one, or one per class)", n_windows,
           K1 - 1);
  TD_CHECK(threshold == threshold && threshold > -__builtin_inf() && hr_threshold == hr_threshold && hr_threshold > -__builtin_inff(),
           "nms_track_seg: thresholds must be numbers above -inf");
  SpotSegArgs a = {};
  for (int i = 0; i < (n_windows == 1 ? 1 : K1 - 1); ++i) {
    TD_CHECK(windows[i] >= soft && windows[i] <= (1 << 30), "nms_track_seg: window %d (soft suppression needs >= 1)", windows[i]);
    a.wl.w[i] = windows[i];
  }
  if (max_len > SPOT_LDS_FRAMES)
    TD_CHECK(workspace && ((uintptr_t)workspace & 7) == 0, "nms_track_seg: a video of %d frames needs an 8-byte aligned workspace of %ld bytes",
             max_len, tdeed_nms_track_seg_workspace(L_total, max_len, K1));
  a.mean = mean; a.seg_off = seg_off; a.nv = nv; a.L_total = L_total; a.max_len = max_len; a.K1 = K1; a.hr = hr_threshold;
  a.thr = threshold; a.soft = soft; a.is_list = n_windows == 1 ? 0 : 1; a.first_frame = first_frame;
  a.ws = (unsigned char*)workspace; a.emitted = emitted; a.kept_score = kept_score; a.st_frame = st_frame;
  a.st_class_u8 = st_class_u8; a.st_score = st_score; a.st_count = st_count; a.rounds = rounds; a.st = (hipStream_t)stream;
  int rc;
  switch (tdeed_nms_track_seg_threads(max_len)) {
    case 128: rc = spot_seg_launch<128>(a); break;
    case 256: rc = spot_seg_launch<256>(a); break;
    case 512: rc = spot_seg_launch<512>(a); break;
    default: rc = spot_seg_launch<SPOT_NT>(a); break;
  }
  if (rc != TDEED_OK) return rc;
  hipLaunchKernelGGL(spot_event_offsets_kernel, dim3(1), dim3(SPOT_NT), 0, a.st, st_count, nv, event_off);
  TD_LAUNCH_CHECK("spot_event_offsets");
  hipLaunchKernelGGL(spot_pack_events_kernel, dim3(nv), dim3(256), 0, a.st, seg_off, L_total, K1, event_off, st_frame, st_class_u8,
                     st_score, out_frame, out_class_u8, out_score);
  TD_LAUNCH_CHECK("spot_pack_events");
  return TDEED_OK;
}
