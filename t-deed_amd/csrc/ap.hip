// Average precision of the spotted events on the device (evalutil.average_precision without the global walk).  Two facts
// make the reference's loop over one globally sorted list parallel (evalutil.ap_match_video / ap_hit_ranks / ap_from_ranks are
// the written statement): whether a prediction recalls a ground-truth frame depends only on the earlier predictions of its own
// class and video, and only the hits need a global position -- which follows from counting, not from sorting the class.
//   ap_match_seg_kernel  one workgroup per (class, video) of a group: compact the events, order them by (score descending, frame
//                        ascending), store them for the rank stage, run the greedy matching once per tolerance (a wave each)
//   ap_rank_kernel       once, after the last group, one workgroup per (entry, tolerance, class): rank of every hit among the
//                        class's predictions of all videos, its position among the hits, precision, running maximum from the
//                        right, sum, / total
// No atomics: every position follows from counts, every sum has one fixed order.
#include "common.h"

#define AP_NT 256                     // threads of both kernels' workgroups
#define AP_NW (AP_NT / WAVE)
#define AP_LDS_FRAMES 8192            // longest video whose events (12 bytes each: score double, frame int32) are ordered in LDS
#define AP_MAX_TOL 8                  // tolerances of one launch (they travel by value in the kernel arguments)
#define AP_GT_LDS_BYTES 49152         // LDS for the ground truth of one (class, video): 4 + n_tol bytes per frame
// 8192 * 12 + 49152 = 147456 bytes of dynamic LDS at most, plus < 1 KiB static: inside the 160 KiB a workgroup may declare.

struct ApTols {
  int t[AP_MAX_TOL];
};

__device__ __forceinline__ int ap_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
  return v;
}

// a precedes b in the matching order: score descending, frame ascending (frames are unique within a class and video)
__device__ __forceinline__ bool ap_before(double sa, int fa, double sb, int fb) { return sa > sb || (sa == sb && fa < fb); }

// =========================================================================== segment + match
// blockIdx.x + 1 = class c, blockIdx.y = video v of the group's packed track (seg_off), ords[v] its ordinal in the dataset
// (index of its name in sorted order).  Events of (c, v): raw (emitted == nullptr): the frames with mean[f][c] >= hr, score
// (double)mean[f][c]; otherwise the frames with emitted[c][f] != 0, score kept_score[c][f] (tdeed_nms_track_seg's planes).
//   1  compaction in frame order (a contiguous run of frames per thread, exclusive scan: positions follow from the flags)
//   2  bitonic network whose comparators all put the earlier element at the lower index; comparators that reach past the n
//      events are skipped, which is the network on the list padded with last-in-order elements (they never move).  IN_LDS: in
//      LDS, then copied out; otherwise in place in the store (same CU, same L1: the workgroup barrier orders the steps)
//   3  store: ev_score / ev_frame [K1-1][LT_all] at vid_off[ord] + i, ev_count [K1-1][NV]
//   4  per tolerance one wave walks the ordered events; the lanes share the open ground-truth frames (entry j belongs to lane
//      j % 64, so a lane alone reads and writes its open flags), key (distance << 32 | index) and a wave minimum give the
//      closest open frame with the first list entry winning ties; a hit closes every entry with that frame; the walk stops
//      when nothing is open.  hit_pos [n_tol][G] at gt_off[ord*K1+c] + k: position i of the k-th hit in the ordered list;
//      hit_count [n_tol][NV*K1].
template <bool IN_LDS>
__global__ __launch_bounds__(AP_NT) void ap_match_seg_kernel(const float* __restrict__ mean, const unsigned char* __restrict__ emitted,
                                                           const double* __restrict__ kept_score, const int* __restrict__ seg_off,
                                                           int L_total, int max_len, int K1, float hr, const int* __restrict__ ords,
                                                           int NV, const int* __restrict__ vid_off, long LT_all,
                                                           const int* __restrict__ gt_off, const int* __restrict__ gt_frames, int G,
                                                           int max_gt, ApTols tols, int n_tol, double* ev_score, int* ev_frame,
                                                           int* __restrict__ ev_count, int* __restrict__ hit_pos,
                                                           int* __restrict__ hit_count) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ap_smem[];
  __shared__ int wave_tot[AP_NW];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c = blockIdx.x + 1;
  const int v = blockIdx.y;
  const int p0 = seg_off[v];
  const int L = seg_off[v + 1] - p0;
  const int ord = ords[v];
  if (p0 < 0 || L <= 0 || L > max_len || (long)p0 + L > L_total || ord < 0 || ord >= NV) return;      // uniform: tables that do
  const int g0 = vid_off[ord];                                                                         // not fit the buffers
  if (g0 < 0 || vid_off[ord + 1] - g0 != L || (long)g0 + L > LT_all) return;
  const int gb = gt_off[(long)ord * K1 + c];
  const int ngt = gt_off[(long)ord * K1 + c + 1] - gb;
  if (gb < 0 || ngt < 0 || ngt > max_gt || (long)gb + ngt > G) return;
  double* const out_s = ev_score + (long)(c - 1) * LT_all + g0;
  int* const out_f = ev_frame + (long)(c - 1) * LT_all + g0;
  double* S;
  int* F;
  unsigned char* gt_base;
  if (IN_LDS) {
    S = reinterpret_cast<double*>(ap_smem);
    F = reinterpret_cast<int*>(ap_smem + (long)max_len * 8);
    gt_base = ap_smem + (long)max_len * 12;
  } else {
    S = out_s;
    F = out_f;
    gt_base = ap_smem;
  }
  int* const gt = reinterpret_cast<int*>(gt_base);
  unsigned char* const open = gt_base + (long)max_gt * 4;
  // ---- 1 compaction
  const bool raw = emitted == nullptr;
  const int per = (L + AP_NT - 1) / AP_NT;
  const int f0 = per * tid < L ? per * tid : L;
  const int f1 = f0 + per < L ? f0 + per : L;
  const float* mcol = mean + (long)p0 * K1 + c;
  const unsigned char* em = raw ? nullptr : emitted + (long)c * L_total + p0;
  const double* ks = raw ? nullptr : kept_score + (long)c * L_total + p0;
  int cnt = 0;
  for (int f = f0; f < f1; ++f) cnt += raw ? (mcol[(long)f * K1] >= hr ? 1 : 0) : (em[f] ? 1 : 0);
  int inc = cnt;
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const int up = __shfl_up(inc, o, WAVE);
    if (lane >= o) inc += up;
  }
  if (lane == 63) wave_tot[wv] = inc;
  __syncthreads();
  int pos = inc - cnt;
  int n = 0;
#pragma unroll
  for (int q = 0; q < AP_NW; ++q) {
    pos += q < wv ? wave_tot[q] : 0;
    n += wave_tot[q];
  }
  for (int f = f0; f < f1; ++f) {
    double s;
    bool on;
    if (raw) {
      const float x = mcol[(long)f * K1];
      on = x >= hr;
      s = (double)x;
    } else {
      on = em[f] != 0;
      s = on ? ks[f] : 0.0;
    }
    if (on) {
      TD_DEV_ASSERT(pos >= 0 && pos < L);
      S[pos] = s;
      F[pos] = f;
      ++pos;
    }
  }
  // the ground truth of (c, v) and every tolerance's open flags
  for (int j = tid; j < ngt; j += AP_NT) gt[j] = gt_frames[gb + j];
  for (int j = tid; j < n_tol * max_gt; j += AP_NT) open[j] = 1;
  __syncthreads();
  // ---- 2 order
  for (int k = 2; (k >> 1) < n; k <<= 1) {
    for (int j = k; j > 0; j = (j == k) ? (k >> 2) : (j >> 1)) {      // j == k: the mirrored step, then distances k/4 .. 1
      for (int i = tid; i < n; i += AP_NT) {
        const int l = (j == k) ? (i ^ (k - 1)) : (i ^ j);
        if (l > i && l < n) {
          const double si = S[i], sl = S[l];
          const int fi = F[i], fl = F[l];
          if (ap_before(sl, fl, si, fi)) {
            S[i] = sl; F[i] = fl;
            S[l] = si; F[l] = fi;
          }
        }
      }
      __syncthreads();
    }
  }
  // ---- 3 store
  if (IN_LDS) {
    for (int i = tid; i < n; i += AP_NT) {
      out_s[i] = S[i];
      out_f[i] = F[i];
    }
  }
  if (tid == 0) ev_count[(long)(c - 1) * NV + ord] = n;
  // ---- 4 matching: wave wv takes the tolerances wv, wv + AP_NW, ...
  for (int ti = wv; ti < n_tol; ti += AP_NW) {
    const unsigned long long tol = (unsigned long long)tols.t[ti];
    unsigned char* op = open + (long)ti * max_gt;
    int* hp = hit_pos + (long)ti * G + gb;
    int n_open = ngt, nh = 0;
    for (int i = 0; i < n && n_open > 0; ++i) {
      const long long f = F[i];
      unsigned long long best = ~0ull;
      for (int j = lane; j < ngt; j += WAVE) {
        if (op[j]) {
          const long long d = (long long)gt[j] - f;
          const unsigned long long key = ((unsigned long long)(d < 0 ? -d : d) << 32) | (unsigned)j;
          best = key < best ? key : best;                             // j ascends: the first entry of a lane wins its ties
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, WAVE);
        best = other < best ? other : best;
      }
      if (best != ~0ull && (best >> 32) <= tol) {                     // uniform
        const int jb = (int)(best & 0xffffffffull);
        TD_DEV_ASSERT(jb >= 0 && jb < ngt && nh < ngt);
        const int hf = gt[jb];
        int closed = 0;
        for (int j = lane; j < ngt; j += WAVE) {
          if (op[j] && gt[j] == hf) {
            op[j] = 0;
            ++closed;
          }
        }
        n_open -= ap_wave_sum(closed);
        if (lane == 0) hp[nh] = i;
        ++nh;
      }
    }
    if (lane == 0) hit_count[(long)ti * NV * K1 + (long)ord * K1 + c] = nh;
  }
}

// =========================================================================== rank + AP
// blockIdx = (class - 1, tolerance, entry).  Videos are ordinals here.  A wave per hit (the waves take the videos in turn),
// the lanes share the videos u it is counted against:
//   A  rank i of hit (v, pos, score s) = 1 + predictions of the class before it in (score descending, video ascending, frame
//      ascending): in video u < v those with score >= s, in u > v those with score > s (binary search in u's ordered list),
//      in v itself pos
//   B  position among the hits by rank: the hits of one video are in ascending rank already, so again a binary search per
//      video; p = (position + 1) / i goes to that position of the class's share of psorted
//   C  running maximum from the right and the sum: a contiguous chunk per thread, the chunks' maxima through LDS, one thread
//      adds the 256 partial sums in index order; AP = sum / total
__global__ __launch_bounds__(AP_NT) void ap_rank_kernel(const double* __restrict__ ev_score, const int* __restrict__ ev_count,
                                                      const int* __restrict__ vid_off, int NV, long LT_all,
                                                      const int* __restrict__ gt_off, int G, int K1, int n_tol,
                                                      const int* __restrict__ hit_pos, const int* __restrict__ hit_count,
                                                      const int* __restrict__ class_off, int* rank, double* psorted,
                                                      double* __restrict__ ap, int* __restrict__ nhits) {
  __shared__ double sh_d[AP_NT];
  __shared__ int sh_i[AP_NW];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c = blockIdx.x + 1, t = blockIdx.y, e = blockIdx.z;
  const double* S = ev_score + ((long)e * (K1 - 1) + (c - 1)) * LT_all;
  const int* cnt = ev_count + ((long)e * (K1 - 1) + (c - 1)) * NV;
  const long et = (long)e * n_tol + t;
  const int* hp = hit_pos + et * G;
  const int* hc = hit_count + et * NV * K1;
  int* rk = rank + et * G;
  const int c0 = class_off[c];
  const int total = class_off[c + 1] - c0;
  double* ps = psorted + et * G + c0;
  // ---- A
  int mine = 0;
  for (int v = wv; v < NV; v += AP_NW) {
    const int nh = hc[(long)v * K1 + c];
    const int gb = gt_off[(long)v * K1 + c];
    if (lane == 0) mine += nh;
    for (int k = 0; k < nh; ++k) {
      const int pos = hp[gb + k];
      const double s = S[vid_off[v] + pos];
      int before = 0;
      for (int u = lane; u < NV; u += WAVE) {
        if (u == v) {
          before += pos;
          continue;
        }
        const double* base = S + vid_off[u];
        int lo = 0, hi = cnt[u];
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          const double x = base[mid];
          if (u < v ? x >= s : x > s) lo = mid + 1; else hi = mid;
        }
        before += lo;
      }
      before = ap_wave_sum(before);
      if (lane == 0) rk[gb + k] = before + 1;
    }
  }
  if (lane == 0) sh_i[wv] = mine;
  __syncthreads();                                                   // also publishes rk[] to the workgroup
  int h = 0;
#pragma unroll
  for (int q = 0; q < AP_NW; ++q) h += sh_i[q];
  TD_DEV_ASSERT(h <= total);
  // ---- B
  for (int v = wv; v < NV; v += AP_NW) {
    const int nh = hc[(long)v * K1 + c];
    const int gb = gt_off[(long)v * K1 + c];
    for (int k = 0; k < nh; ++k) {
      const int r = rk[gb + k];
      int less = 0;
      for (int u = lane; u < NV; u += WAVE) {
        if (u == v) {
          less += k;
          continue;
        }
        const int* base = rk + gt_off[(long)u * K1 + c];
        int lo = 0, hi = hc[(long)u * K1 + c];
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (base[mid] < r) lo = mid + 1; else hi = mid;
        }
        less += lo;
      }
      less = ap_wave_sum(less);
      TD_DEV_ASSERT(less < h);
      if (lane == 0) ps[less] = (double)(less + 1) / (double)r;      // correctly rounded: no fast-math in this build
    }
  }
  __syncthreads();
  // ---- C
  const int per = (h + AP_NT - 1) / AP_NT;
  const int a = per * tid < h ? per * tid : h;
  const int b = a + per < h ? a + per : h;
  double m = 0.0;
  for (int j = a; j < b; ++j) m = fmax(m, ps[j]);
  sh_d[tid] = m;
  __syncthreads();
  double run = 0.0;
  for (int q = tid + 1; q < AP_NT; ++q) run = fmax(run, sh_d[q]);
  __syncthreads();
  double sum = 0.0;
  for (int j = b - 1; j >= a; --j) {
    run = fmax(run, ps[j]);
    sum += run;
  }
  sh_d[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    for (int q = 0; q < AP_NT; ++q) tot += sh_d[q];
    ap[et * K1 + c] = (h > 0 && total > 0) ? tot / (double)total : 0.0;
    nhits[et * K1 + c] = h;
    if (c == 1) {
      ap[et * K1] = 0.0;                                             // the background column has no events
      nhits[et * K1] = 0;
    }
  }
}

// =========================================================================== exchange of the state between ranks
// A validation pass sharded over ranks leaves every rank with the segments of its own videos.  After the counts have been
// summed over the ranks (ev_count / hit_count are zero where a rank filled nothing), the used part of every segment has a
// place in a dense payload: the exclusive scan of the counts in the store's own order -- (e, c, ord) for the scores, (e, t,
// ord*K1+c) for the hits.  PACK copies the rank's own segments out of the stores into the (zero-filled) payloads, !PACK
// writes the foreign segments of the summed payloads into the stores: one body, the copy turned round.
//   One thread per payload element; it finds its segment by a binary search in the inclusive scan (sc_end / hc_end, int64, in
// global memory: the E*(K1-1)*NV + E*T*NV*K1 entries do not fit LDS in general, but a wave's 64 consecutive elements walk the
// same few cache lines of it).  The work is the payload, whatever the sizes of the segments: a workgroup per segment would
// leave most workgroups empty (most (class, video) pairs of a tolerance have no hit) and a few with thousands of elements.
// Empty segments are skipped by the search itself (their end equals their predecessor's).  The first blocks_s workgroups take
// the score payload (8-byte elements), the others the hit payload (4-byte elements).  No atomics, no LDS, no scratch.
template <bool PACK>
__global__ __launch_bounds__(AP_NT) void ap_state_xchg_kernel(double* ev_score, int* hit_pos, double* pay_s, int* pay_h,
                                                            const long* __restrict__ sc_end, const long* __restrict__ hc_end,
                                                            long n_s, long n_h, long nseg_s, long nseg_h, int blocks_s,
                                                            const int* __restrict__ own, const int* __restrict__ vid_off,
                                                            const int* __restrict__ gt_off, int NV, int K1, long LT_all,
                                                            long hit_stride) {
  const bool scores = (int)blockIdx.x < blocks_s;
  const long i = (long)(scores ? blockIdx.x : blockIdx.x - blocks_s) * AP_NT + threadIdx.x;
  const long n = scores ? n_s : n_h;
  if (i >= n) return;
  const long* __restrict__ end = scores ? sc_end : hc_end;
  long lo = 0, hi = scores ? nseg_s : nseg_h;                          // the first segment whose end lies beyond i
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (end[mid] <= i) lo = mid + 1; else hi = mid;
  }
  const long s = lo;
  if (s >= (scores ? nseg_s : nseg_h)) return;                         // a payload longer than the scan says: not followed
  const long k = i - (s > 0 ? end[s - 1] : 0);                         // position inside the segment
  if (k < 0) return;
  if (scores) {
    const long row = s / NV;                                           // e * (K1-1) + c - 1
    const int ord = (int)(s - row * NV);
    const long g0 = vid_off[ord];
    if (g0 < 0 || g0 + k >= (long)vid_off[ord + 1] || g0 + k >= LT_all) return;      // a count beyond the video's frames
    const long j = row * LT_all + g0 + k;
    if (PACK) {
      if (own[ord]) pay_s[i] = ev_score[j];
    } else {
      if (!own[ord]) ev_score[j] = pay_s[i];
    }
  } else {
    const long nk = (long)NV * K1;
    const long row = s / nk;                                           // e * n_tol + t
    const long oc = s - row * nk;                                      // ord * K1 + c
    const int ord = (int)(oc / K1);
    const long g0 = gt_off[oc];
    if (g0 < 0 || g0 + k >= (long)gt_off[oc + 1] || g0 + k >= hit_stride) return;      // more hits than ground-truth frames
    const long j = row * hit_stride + g0 + k;
    if (PACK) {
      if (own[ord]) pay_h[i] = hit_pos[j];
    } else {
      if (!own[ord]) hit_pos[j] = pay_h[i];
    }
  }
}

static int ap_state_xchg(bool pack, double* ev_score, int* hit_pos, double* pay_s, int* pay_h, const long* sc_end,
                         const long* hc_end, long n_s, long n_h, const int* own, const int* vid_off, const int* gt_off, int NV,
                         int K1, int n_entries, int n_tol, long LT_all, int G, void* stream) {
  const char* who = pack ? "ap_state_pack" : "ap_state_unpack";
  TD_CHECK(ev_score && hit_pos && sc_end && hc_end && own && vid_off && gt_off, "%s: null pointer", who);
  TD_CHECK(NV > 0 && LT_all > 0 && LT_all < (1l << 31) && K1 > 1 && K1 <= 256 && G >= 0 && (long)NV * K1 < (1l << 31), "%s: bad sizes", who);
  TD_CHECK(n_entries >= 1 && n_entries <= 65535 && n_tol >= 1 && n_tol <= AP_MAX_TOL, "%s: %d entries, %d tolerances", who,
           n_entries, n_tol);
  TD_CHECK(n_s >= 0 && n_h >= 0 && (n_s == 0 || pay_s) && (n_h == 0 || pay_h), "%s: payloads of %ld / %ld elements", who, n_s, n_h);
  TD_CHECK(n_s <= (long)n_entries * (K1 - 1) * LT_all && n_h <= (long)n_entries * n_tol * (G > 0 ? G : 1),
           "%s: payloads of %ld / %ld elements are larger than the stores", who, n_s, n_h);
  const long bs = (n_s + AP_NT - 1) / AP_NT, bh = (n_h + AP_NT - 1) / AP_NT;
  TD_CHECK(bs + bh < (1l << 31), "%s: %ld workgroups", who, bs + bh);
  if (bs + bh == 0) return TDEED_OK;
  const long nseg_s = (long)n_entries * (K1 - 1) * NV, nseg_h = (long)n_entries * n_tol * NV * K1;
  auto kernel = pack ? ap_state_xchg_kernel<true> : ap_state_xchg_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(bs + bh)), dim3(AP_NT), 0, (hipStream_t)stream, ev_score, hit_pos, pay_s, pay_h, sc_end,
                     hc_end, n_s, n_h, nseg_s, nseg_h, (int)bs, own, vid_off, gt_off, NV, K1, LT_all, (long)(G > 0 ? G : 1));
  TD_LAUNCH_CHECK(who);
  return TDEED_OK;
}

// =========================================================================== C entries
extern "C" int tdeed_ap_state_pack(const double* ev_score, const int* hit_pos, double* scores, int* hits, const long* sc_end,
                                   const long* hc_end, long n_scores, long n_hits, const int* own, const int* vid_off,
                                   const int* gt_off, int NV, int K1, int n_entries, int n_tol, long LT_all, int G, void* stream) {
  return ap_state_xchg(true, const_cast<double*>(ev_score), const_cast<int*>(hit_pos), scores, hits, sc_end, hc_end, n_scores,
                       n_hits, own, vid_off, gt_off, NV, K1, n_entries, n_tol, LT_all, G, stream);
}

extern "C" int tdeed_ap_state_unpack(double* ev_score, int* hit_pos, const double* scores, const int* hits, const long* sc_end,
                                     const long* hc_end, long n_scores, long n_hits, const int* own, const int* vid_off,
                                     const int* gt_off, int NV, int K1, int n_entries, int n_tol, long LT_all, int G, void* stream) {
  return ap_state_xchg(false, ev_score, hit_pos, const_cast<double*>(scores), const_cast<int*>(hits), sc_end, hc_end, n_scores,
                       n_hits, own, vid_off, gt_off, NV, K1, n_entries, n_tol, LT_all, G, stream);
}

extern "C" int tdeed_ap_lds_frames(void) { return AP_LDS_FRAMES; }
extern "C" int tdeed_ap_max_tolerances(void) { return AP_MAX_TOL; }
extern "C" int tdeed_ap_max_truth(int n_tol) { return n_tol >= 1 && n_tol <= AP_MAX_TOL ? AP_GT_LDS_BYTES / (4 + n_tol) : 0; }

extern "C" int tdeed_ap_match_seg(const float* mean, const unsigned char* emitted, const double* kept_score, const int* seg_off,
                                  int nv, int L_total, int max_len, int K1, float hr_threshold, const int* ords, int NV,
                                  const int* vid_off, long LT_all, const int* gt_off, const int* gt_frames, int G, int max_gt,
                                  const int* tolerances, int n_tol, double* ev_score, int* ev_frame, int* ev_count, int* hit_pos,
                                  int* hit_count, void* stream) {
  TD_CHECK(mean && seg_off && ords && vid_off && gt_off && gt_frames && tolerances && ev_score && ev_frame && ev_count && hit_pos &&
               hit_count,
           "ap_match_seg: null pointer");
  TD_CHECK((emitted == nullptr) == (kept_score == nullptr), "ap_match_seg: emitted and kept_score go together");
  TD_CHECK(L_total > 0 && K1 > 1 && nv > 0 && max_len > 0 && max_len <= L_total, "ap_match_seg: bad sizes");
  TD_CHECK(nv <= 65535 && K1 <= 256, "ap_match_seg: %d videos in one group (at most 65535), %d columns (at most 256)", nv, K1);
  TD_CHECK(NV >= nv && LT_all >= L_total && LT_all < (1l << 31), "ap_match_seg: a dataset of %d videos and %ld frames for a group of %d / %d",
           NV, LT_all, nv, L_total);
  TD_CHECK((long)NV * K1 < (1l << 31) && G >= 0, "ap_match_seg: bad truth table");
  TD_CHECK(n_tol >= 1 && n_tol <= AP_MAX_TOL, "ap_match_seg: %d tolerances, 1 to %d", n_tol, AP_MAX_TOL);
  TD_CHECK(max_gt >= 0 && max_gt <= tdeed_ap_max_truth(n_tol),
           "ap_match_seg: %d ground-truth frames in one (class, video), at most %d with %d tolerances", max_gt,
           tdeed_ap_max_truth(n_tol), n_tol);
  TD_CHECK(hr_threshold == hr_threshold, "ap_match_seg: the threshold must be a number");
  ApTols tl = {};
  for (int i = 0; i < n_tol; ++i) {
    TD_CHECK(tolerances[i] >= 0, "ap_match_seg: tolerance %d", tolerances[i]);
    tl.t[i] = tolerances[i];
  }
  hipStream_t st = (hipStream_t)stream;
  const bool in_lds = max_len <= AP_LDS_FRAMES;
  const size_t gt_bytes = ((size_t)max_gt * (4 + n_tol) + 15) & ~(size_t)15;
  const size_t lds = (in_lds ? (size_t)max_len * 12 : 0) + gt_bytes;
  auto kernel = in_lds ? ap_match_seg_kernel<true> : ap_match_seg_kernel<false>;
  if (lds > 32768) {                                               // beyond what a launch may ask for without the attribute
    static TdDevOnce once[2];
    if (!once[in_lds].get()) {
      hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (in_lds ? AP_LDS_FRAMES * 12 : 0) + AP_GT_LDS_BYTES + 16);
      if (e != hipSuccess) { tdeed_set_error("ap_match_seg: hipFuncSetAttribute: %s", hipGetErrorString(e)); return TDEED_ERR_RUNTIME; }
      once[in_lds].set();
    }
  }
  hipLaunchKernelGGL(kernel, dim3(K1 - 1, nv), dim3(AP_NT), lds, st, mean, emitted, kept_score, seg_off, L_total, max_len, K1,
                     hr_threshold, ords, NV, vid_off, LT_all, gt_off, gt_frames, G, max_gt, tl, n_tol, ev_score, ev_frame, ev_count,
                     hit_pos, hit_count);
  TD_LAUNCH_CHECK("ap_match_seg");
  return TDEED_OK;
}

extern "C" int tdeed_ap_rank(const double* ev_score, const int* ev_count, const int* vid_off, int NV, long LT_all, const int* gt_off,
                             int G, int K1, int n_entries, int n_tol, const int* hit_pos, const int* hit_count, const int* class_off,
                             int* rank, double* psorted, double* ap, int* nhits, void* stream) {
  TD_CHECK(ev_score && ev_count && vid_off && gt_off && hit_pos && hit_count && class_off && rank && psorted && ap && nhits,
           "ap_rank: null pointer");
  TD_CHECK(NV > 0 && LT_all > 0 && LT_all < (1l << 31) && K1 > 1 && K1 <= 256 && G >= 0 && (long)NV * K1 < (1l << 31), "ap_rank: bad sizes");
  TD_CHECK(n_entries >= 1 && n_entries <= 65535, "ap_rank: %d entries", n_entries);
  TD_CHECK(n_tol >= 1 && n_tol <= AP_MAX_TOL, "ap_rank: %d tolerances, 1 to %d", n_tol, AP_MAX_TOL);
  hipLaunchKernelGGL(ap_rank_kernel, dim3(K1 - 1, n_tol, n_entries), dim3(AP_NT), 0, (hipStream_t)stream, ev_score, ev_count, vid_off, NV,
                     LT_all, gt_off, G, K1, n_tol, hit_pos, hit_count, class_off, rank, psorted, ap, nhits);
  TD_LAUNCH_CHECK("ap_rank");
  return TDEED_OK;
}
