// First pieces of the training path: the output end of the backward chain
// and the optimizer.  Loss backward (weighted CE hard/soft + MSE, reference model/model.py:308-319), heads
// backward (FCLayers, model/modules.py:366-376) and a fused multi-tensor AdamW over one flat fp32 buffer
// (BaseRGBModel.get_optimizer -> torch.optim.AdamW defaults, model/modules.py:37-39).
#include "common.h"

// ------------------------------------------------------------------------------------------ loss backward
// d(total)/d(head_out) for head_out [rows][ld] (columns [0,K1) logits, column displ_col the displacement).
//   hard labels: dlogit[r][k] = w[y_r] (softmax_rk - [k==y_r]) / sum_r w[y_r]
//   soft labels: dlogit[r][k] = (softmax_rk * sum_c w_c p_rc - w_k p_rk) / rows
//   MSE:         ddispl[r]    = 2 (d_r - labelD_r) / rows
// single block (rows = B*T is a few thousand); columns outside the loss get zero gradient.
__global__ __launch_bounds__(256) void loss_bwd_kernel(const float* __restrict__ head, int rows, int ld, int K1,
                                                       const int64_t* __restrict__ hard,
                                                       const float* __restrict__ soft,
                                                       const float* __restrict__ cls_w, int displ_col,
                                                       const float* __restrict__ labelD, float gscale,
                                                       float* __restrict__ dhead) {
  __shared__ float scratch[8];
  float den = 0.f;
  if (!soft)
    for (int r = threadIdx.x; r < rows; r += 256) {
      const int y = (int)hard[r];
      den += cls_w[(y >= 0 && y < K1) ? y : 0];                  // out-of-range labels are never indexed (tdeed_loss_fwd -> NaN)
    }
  den = soft ? (float)rows : block_sum<4>(den, scratch);
  const float inv = gscale / den;
  for (int r = threadIdx.x; r < rows; r += 256) {
    const float* lg = head + (long)r * ld;
    float* dg = dhead + (long)r * ld;
    float m = lg[0];
    for (int k = 1; k < K1; ++k) m = fmaxf(m, lg[k]);
    float s = 0.f;
    for (int k = 0; k < K1; ++k) s += expf(lg[k] - m);
    const float is = 1.0f / s;
    for (int k = K1; k < ld; ++k) dg[k] = 0.f;
    if (soft) {
      const float* p = soft + (long)r * K1;
      float wp = 0.f;
      for (int k = 0; k < K1; ++k) wp += cls_w[k] * p[k];
      for (int k = 0; k < K1; ++k) dg[k] = (expf(lg[k] - m) * is * wp - cls_w[k] * p[k]) * inv;
    } else {
      int y = (int)hard[r];
      if (y < 0 || y >= K1) y = 0;
      const float wy = cls_w[y];
      for (int k = 0; k < K1; ++k) dg[k] = wy * (expf(lg[k] - m) * is - (k == y ? 1.f : 0.f)) * inv;
    }
    if (displ_col >= 0 && labelD) dg[displ_col] = 2.0f * (lg[displ_col] - labelD[r]) * gscale / (float)rows;
  }
}

extern "C" int tdeed_loss_bwd(const float* head_out, int rows, int ld, int K1, const int64_t* hard, const float* soft,
                              const float* cls_w, int displ_col, const float* labelD, float grad_scale,
                              float* dhead, void* stream) {
  TD_CHECK(head_out && cls_w && dhead && (hard || soft), "loss_bwd: null pointer");
  TD_CHECK(rows > 0 && K1 > 0 && K1 <= ld && displ_col < ld, "loss_bwd: bad sizes");
  hipLaunchKernelGGL(loss_bwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, head_out, rows, ld, K1, hard, soft,
                     cls_w, displ_col, labelD, grad_scale, dhead);
  TD_LAUNCH_CHECK("loss_bwd");
  return TDEED_OK;
}

// ------------------------------------------------------------------------------------------ distillation loss
// Value and gradient of  total = (1-a) CE + MSE + a KD + b KDdispl  in one launch (opt-in: TDEEDModel.distill_from).
//   CE, MSE:  the terms of loss_kernel (misc.hip) / loss_bwd_kernel above, expression for expression, so that a = b = 0
//             gives their bits
//   KD      = tau^2 / rows * sum_r sum_k q_rk (log q_rk - log p_rk),  p = softmax(s_r / tau), q = softmax(t_r / tau);
//             s = head[r][0..K1), t = teacher[r][0..K1) read in place from the teacher's head buffer (row stride ld_t)
//   KDdispl = 1 / rows * sum_r (d_s - d_t)^2  when both heads have a displacement column, else 0
//   dlogit[r][k] = (1-a) (the plain term) + a tau (p_rk - q_rk) gscale / rows
//   ddispl[r]    = the plain term + 2 b (d_s - d_t) gscale / rows
// Single block like the kernels it restates; every thread walks its rows in order and the block folds are fixed trees:
// no atomics, the same bits at every launch.  Per row the two tempered softmaxes are reduced once (max, sum, log-sum) and
// serve the value and the gradient.  Nothing is clamped: a non-finite teacher logit reaches KD and that row's gradient
// (the guarded step's skip_nonfinite is what catches it).
__global__ __launch_bounds__(256) void loss_kd_kernel(const float* __restrict__ head, int rows, int ld, int K1,
                                                      const int64_t* __restrict__ hard, const float* __restrict__ soft,
                                                      const float* __restrict__ cls_w, int displ_col,
                                                      const float* __restrict__ labelD,
                                                      const float* __restrict__ teacher, int ld_t, int displ_col_t,
                                                      float alpha, float tau, float beta, float gscale,
                                                      float* __restrict__ out, float* __restrict__ dhead) {
  __shared__ float scratch[8];
  float den = 0.f;
  if (!soft)
    for (int r = threadIdx.x; r < rows; r += 256) {
      const int y = (int)hard[r];
      den += cls_w[(y >= 0 && y < K1) ? y : 0];                  // out-of-range labels are never indexed
    }
  den = soft ? (float)rows : block_sum<4>(den, scratch);
  const float inv = gscale / den;
  const float oma = 1.0f - alpha;
  const float it = 1.0f / tau;
  const float gk = alpha * tau * gscale / (float)rows;
  const float gd = 2.0f * beta * gscale / (float)rows;
  const bool both_d = displ_col >= 0 && displ_col_t >= 0;
  float num = 0.f, se = 0.f, bad = 0.f, kd = 0.f, kdd = 0.f;
  for (int r = threadIdx.x; r < rows; r += 256) {
    const float* lg = head + (long)r * ld;
    const float* tg = teacher + (long)r * ld_t;
    float m = lg[0], mt = tg[0];
    for (int k = 1; k < K1; ++k) { m = fmaxf(m, lg[k]); mt = fmaxf(mt, tg[k]); }
    float s = 0.f;
    for (int k = 0; k < K1; ++k) s += expf(lg[k] - m);
    const float lse = m + logf(s);
    const float is = 1.0f / s;
    // the tempered pair: x -> x / tau is monotone, so the row maxima carry over
    const float ms = m * it;
    mt *= it;
    float ss = 0.f, st = 0.f;
    for (int k = 0; k < K1; ++k) { ss += expf(lg[k] * it - ms); st += expf(tg[k] * it - mt); }
    const float lss = ms + logf(ss), lst = mt + logf(st);
    const float ips = 1.0f / ss, ipt = 1.0f / st;
    if (soft) {
      const float* p = soft + (long)r * K1;
      float a = 0.f;
      for (int k = 0; k < K1; ++k) a += cls_w[k] * p[k] * (lse - lg[k]);
      num += a;
    } else {
      int yk = (int)hard[r];
      if (yk < 0 || yk >= K1) { bad = 1.f; yk = 0; }
      num += cls_w[yk] * (lse - lg[yk]);
    }
    float* dg = dhead ? dhead + (long)r * ld : nullptr;
    if (dg) {
      // the plain term first, in loss_bwd_kernel's own loops (its contractions decide the bits), then blended in place
      for (int k = K1; k < ld; ++k) dg[k] = 0.f;
      if (soft) {
        const float* p = soft + (long)r * K1;
        float wp = 0.f;
        for (int k = 0; k < K1; ++k) wp += cls_w[k] * p[k];
        for (int k = 0; k < K1; ++k) dg[k] = (expf(lg[k] - m) * is * wp - cls_w[k] * p[k]) * inv;
      } else {
        int y = (int)hard[r];
        if (y < 0 || y >= K1) y = 0;
        const float wy = cls_w[y];
        for (int k = 0; k < K1; ++k) dg[k] = wy * (expf(lg[k] - m) * is - (k == y ? 1.f : 0.f)) * inv;
      }
    }
    float a = 0.f;
    for (int k = 0; k < K1; ++k) {
      const float ps = expf(lg[k] * it - ms) * ips, qt = expf(tg[k] * it - mt) * ipt;
      a += qt * ((tg[k] * it - lst) - (lg[k] * it - lss));
      if (dg) dg[k] = oma * dg[k] + gk * (ps - qt);
    }
    kd += a;
    float gdis = 0.f;
    if (displ_col >= 0 && labelD) {
      const float d = lg[displ_col] - labelD[r];
      se += d * d;
      gdis = 2.0f * (lg[displ_col] - labelD[r]) * gscale / (float)rows;
    }
    if (both_d) {
      const float e = lg[displ_col] - tg[displ_col_t];
      kdd += e * e;
      gdis += gd * e;
    }
    if (dg && displ_col >= 0 && (labelD || both_d)) dg[displ_col] = gdis;
  }
  num = block_sum<4>(num, scratch);
  se = block_sum<4>(se, scratch);
  bad = block_sum<4>(bad, scratch);
  kd = block_sum<4>(kd, scratch);
  kdd = block_sum<4>(kdd, scratch);
  if (threadIdx.x == 0) {
    const float ce = bad > 0.f ? __builtin_nanf("") : (soft ? num / (float)rows : num / den);
    const float mse = (displ_col >= 0 && labelD) ? se / (float)rows : 0.f;
    const float kdv = tau * tau * kd / (float)rows;
    const float kddv = both_d ? kdd / (float)rows : 0.f;
    out[0] = oma * ce + mse + alpha * kdv + beta * kddv;
    out[1] = ce;
    out[2] = mse;
    out[3] = kdv;
    out[4] = kddv;
  }
}

extern "C" int tdeed_loss_kd(const float* head_out, int rows, int ld, int K1, const int64_t* hard, const float* soft,
                             const float* cls_w, int displ_col, const float* labelD, const float* teacher, int ld_t,
                             int displ_col_t, float alpha, float temperature, float displ_weight, float grad_scale,
                             float* out5, float* dhead, void* stream) {
  TD_CHECK(head_out && cls_w && teacher && out5 && (hard || soft), "loss_kd: null pointer");
  TD_CHECK(rows > 0 && K1 > 0 && K1 <= ld && displ_col < ld && K1 <= ld_t && displ_col_t < ld_t, "loss_kd: bad sizes");
  TD_CHECK(alpha >= 0.f && alpha <= 1.f && temperature > 0.f && displ_weight >= 0.f, "loss_kd: bad alpha / temperature / weight");
  TD_CHECK(displ_weight == 0.f || (displ_col >= 0 && displ_col_t >= 0), "loss_kd: displ_weight without both displacement columns");
  hipLaunchKernelGGL(loss_kd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, head_out, rows, ld, K1, hard, soft,
                     cls_w, displ_col, labelD, teacher, ld_t, displ_col_t, alpha, temperature, displ_weight, grad_scale,
                     out5, dhead);
  TD_LAUNCH_CHECK("loss_kd");
  return TDEED_OK;
}

// ------------------------------------------------------------------------------------------ loss options
// Label smoothing eps, focal exponent gamma and free per-class weights w on the classification term, value and gradient in
// one launch (opt-in: TDEEDModel.loss_options); with a teacher the distillation terms of loss_kd_kernel on top:
//   total = (1-a) CE + MSE + a KD + b KDdispl,   MSE / KD / KDdispl and their gradients exactly loss_kd_kernel's.
// Per row with logits s:  lse = m + log sum exp(s - m),  logp_c = s_c - lse  (never the log of a rounded probability),
//   p_c = exp(logp_c),  q_c = 1 - p_c = -expm1(logp_c),  t'_c = (1-eps) t_c + eps / K1  (t: one-hot or the soft row),
//   a_c = w_c t'_c,
//   CE  = sum_r sum_c a_c q_c^gamma (-logp_c) / den,   den = sum_r w[y_r] (hard) or rows (soft): torch's rule
//   g_c = -a_c q_c^gamma (gamma p_c rho_c + 1),  rho_c = -logp_c / q_c where q_c > 0, else 1 (its limit)
//   dlogit_k = (g_k - p_k sum_c g_c) gscale / den
// The rho form keeps a saturated row (p_y == 1 in fp32: logp = 0, q = 0) finite for every gamma: q^(gamma-1) never
// appears.  Terms with a_c == 0 are skipped, at gamma == 0 powf is not called, nothing is clamped.  g_k waits in dhead
// between the two class passes (written and read by the same thread).
// eps == gamma == 0 takes loss_kernel's / loss_bwd_kernel's own loops on a uniform branch: their bits, and with a teacher
// loss_kd_kernel's.  Single block, fixed fold order, no atomics.
__global__ __launch_bounds__(256) void loss_opt_kernel(const float* __restrict__ head, int rows, int ld, int K1,
                                                       const int64_t* __restrict__ hard, const float* __restrict__ soft,
                                                       const float* __restrict__ cls_w, int displ_col,
                                                       const float* __restrict__ labelD,
                                                       const float* __restrict__ teacher, int ld_t, int displ_col_t,
                                                       float alpha, float tau, float beta, float eps, float gamma,
                                                       float gscale, float* __restrict__ out, float* __restrict__ dhead) {
  __shared__ float scratch[8];
  float den = 0.f;
  if (!soft)
    for (int r = threadIdx.x; r < rows; r += 256) {
      const int y = (int)hard[r];
      den += cls_w[(y >= 0 && y < K1) ? y : 0];                  // out-of-range labels are never indexed
    }
  den = soft ? (float)rows : block_sum<4>(den, scratch);
  const float inv = gscale / den;
  const float oma = 1.0f - alpha;
  const float it = 1.0f / tau;
  const float gk = alpha * tau * gscale / (float)rows;
  const float gd = 2.0f * beta * gscale / (float)rows;
  const bool kdon = teacher != nullptr;
  const bool both_d = kdon && displ_col >= 0 && displ_col_t >= 0;
  const bool neutral = eps == 0.f && gamma == 0.f;
  const float ome = 1.0f - eps, eu = eps / (float)K1;
  float num = 0.f, se = 0.f, bad = 0.f, kd = 0.f, kdd = 0.f;
  for (int r = threadIdx.x; r < rows; r += 256) {
    const float* lg = head + (long)r * ld;
    float m = lg[0];
    for (int k = 1; k < K1; ++k) m = fmaxf(m, lg[k]);
    float s = 0.f;
    for (int k = 0; k < K1; ++k) s += expf(lg[k] - m);
    const float lse = m + logf(s);
    const float is = 1.0f / s;
    float* dg = dhead ? dhead + (long)r * ld : nullptr;
    if (dg)
      for (int k = K1; k < ld; ++k) dg[k] = 0.f;
    if (neutral) {
      if (soft) {
        const float* p = soft + (long)r * K1;
        float a = 0.f;
        for (int k = 0; k < K1; ++k) a += cls_w[k] * p[k] * (lse - lg[k]);
        num += a;
      } else {
        int yk = (int)hard[r];
        if (yk < 0 || yk >= K1) { bad = 1.f; yk = 0; }
        num += cls_w[yk] * (lse - lg[yk]);
      }
      if (dg) {
        if (soft) {
          const float* p = soft + (long)r * K1;
          float wp = 0.f;
          for (int k = 0; k < K1; ++k) wp += cls_w[k] * p[k];
          for (int k = 0; k < K1; ++k) dg[k] = (expf(lg[k] - m) * is * wp - cls_w[k] * p[k]) * inv;
        } else {
          int y = (int)hard[r];
          if (y < 0 || y >= K1) y = 0;
          const float wy = cls_w[y];
          for (int k = 0; k < K1; ++k) dg[k] = wy * (expf(lg[k] - m) * is - (k == y ? 1.f : 0.f)) * inv;
        }
      }
    } else {
      const float* p = soft ? soft + (long)r * K1 : nullptr;
      int y = 0;
      if (!soft) {
        y = (int)hard[r];
        if (y < 0 || y >= K1) { bad = 1.f; y = 0; }
      }
      float a = 0.f, gsum = 0.f;
      for (int k = 0; k < K1; ++k) {
        const float t = p ? p[k] : (k == y ? 1.f : 0.f);
        const float ak = cls_w[k] * (ome * t + eu);
        float g = 0.f;
        if (ak != 0.f) {
          const float logp = lg[k] - lse;
          float f = ak, h = 1.f;                                   // a q^gamma,  gamma p rho + 1
          if (gamma != 0.f) {
            const float q = -expm1f(logp);
            const float rho = q > 0.f ? -logp / q : 1.f;
            f = ak * powf(q, gamma);
            h = gamma * expf(logp) * rho + 1.f;
          }
          a -= f * logp;
          g = -f * h;
        }
        gsum += g;
        if (dg) dg[k] = g;
      }
      num += a;
      if (dg)
        for (int k = 0; k < K1; ++k) dg[k] = (dg[k] - expf(lg[k] - lse) * gsum) * inv;
    }
    if (kdon) {
      const float* tg = teacher + (long)r * ld_t;
      float mt = tg[0];
      for (int k = 1; k < K1; ++k) mt = fmaxf(mt, tg[k]);
      // the tempered pair: x -> x / tau is monotone, so the row maxima carry over
      const float ms = m * it;
      mt *= it;
      float ss = 0.f, st = 0.f;
      for (int k = 0; k < K1; ++k) { ss += expf(lg[k] * it - ms); st += expf(tg[k] * it - mt); }
      const float lss = ms + logf(ss), lst = mt + logf(st);
      const float ips = 1.0f / ss, ipt = 1.0f / st;
      float a = 0.f;
      for (int k = 0; k < K1; ++k) {
        const float ps = expf(lg[k] * it - ms) * ips, qt = expf(tg[k] * it - mt) * ipt;
        a += qt * ((tg[k] * it - lst) - (lg[k] * it - lss));
        if (dg) dg[k] = oma * dg[k] + gk * (ps - qt);
      }
      kd += a;
    }
    float gdis = 0.f;
    if (displ_col >= 0 && labelD) {
      const float d = lg[displ_col] - labelD[r];
      se += d * d;
      gdis = 2.0f * (lg[displ_col] - labelD[r]) * gscale / (float)rows;
    }
    if (both_d) {
      const float e = lg[displ_col] - teacher[(long)r * ld_t + displ_col_t];
      kdd += e * e;
      gdis += gd * e;
    }
    if (dg && displ_col >= 0 && (labelD || both_d)) dg[displ_col] = gdis;
  }
  num = block_sum<4>(num, scratch);
  se = block_sum<4>(se, scratch);
  bad = block_sum<4>(bad, scratch);
  kd = block_sum<4>(kd, scratch);
  kdd = block_sum<4>(kdd, scratch);
  if (threadIdx.x == 0) {
    const float ce = bad > 0.f ? __builtin_nanf("") : (soft ? num / (float)rows : num / den);
    const float mse = (displ_col >= 0 && labelD) ? se / (float)rows : 0.f;
    const float kdv = kdon ? tau * tau * kd / (float)rows : 0.f;
    const float kddv = both_d ? kdd / (float)rows : 0.f;
    out[0] = kdon ? oma * ce + mse + alpha * kdv + beta * kddv : ce + mse;
    out[1] = ce;
    out[2] = mse;
    out[3] = kdv;
    out[4] = kddv;
  }
}

extern "C" int tdeed_loss_opt(const float* head_out, int rows, int ld, int K1, const int64_t* hard, const float* soft,
                              const float* cls_w, int displ_col, const float* labelD, const float* teacher, int ld_t,
                              int displ_col_t, float alpha, float temperature, float displ_weight, float label_smoothing,
                              float focal_gamma, float grad_scale, float* out5, float* dhead, void* stream) {
  TD_CHECK(head_out && cls_w && out5 && (hard || soft), "loss_opt: null pointer");
  TD_CHECK(rows > 0 && K1 > 0 && K1 <= ld && displ_col < ld, "loss_opt: bad sizes");
  TD_CHECK(label_smoothing >= 0.f && label_smoothing <= 1.f, "loss_opt: label_smoothing %g outside [0, 1]", (double)label_smoothing);
  TD_CHECK(focal_gamma >= 0.f && focal_gamma <= 3.0e38f, "loss_opt: focal_gamma %g (non-negative and finite)", (double)focal_gamma);
  if (teacher) {
    TD_CHECK(K1 <= ld_t && displ_col_t < ld_t, "loss_opt: bad teacher sizes");
    TD_CHECK(alpha >= 0.f && alpha <= 1.f && temperature > 0.f && displ_weight >= 0.f, "loss_opt: bad alpha / temperature / weight");
    TD_CHECK(displ_weight == 0.f || (displ_col >= 0 && displ_col_t >= 0), "loss_opt: displ_weight without both displacement columns");
  } else {
    TD_CHECK(alpha == 0.f && displ_weight == 0.f, "loss_opt: alpha / displ_weight without a teacher");
    temperature = 1.0f;
  }
  hipLaunchKernelGGL(loss_opt_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, head_out, rows, ld, K1, hard, soft,
                     cls_w, displ_col, labelD, teacher, ld_t, displ_col_t, alpha, temperature, displ_weight,
                     label_smoothing, focal_gamma, grad_scale, out5, dhead);
  TD_LAUNCH_CHECK("loss_opt");
  return TDEED_OK;
}

// ------------------------------------------------------------------------------------------ heads backward
// out = x W^T + b (x [rows][C] in T, W fp32 [n_out][C]):  dx = dout W (written in T),
// dW[o][c] = sum_r dout[r][o] x[r][c], db[o] = sum_r dout[r][o]   (fp32, deterministic two-stage reduction).
template <typename T>
__global__ __launch_bounds__(256) void heads_bwd_dx_kernel(const float* __restrict__ dout, int rows, int C,
                                                           const float* __restrict__ w, int n_out,
                                                           T* __restrict__ dx) {
  constexpr int EPC = Chunk<T>::N;
  const int cpr = C / EPC;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < (long)rows * cpr; i += (long)gridDim.x * 256) {
    const long r = i / cpr;
    const int c0 = (int)(i - r * cpr) * EPC;
    float a[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) a[e] = 0.f;
    for (int o = 0; o < n_out; ++o) {
      const float g = dout[r * n_out + o];
#pragma unroll
      for (int e = 0; e < EPC; ++e) a[e] = fmaf(g, w[(long)o * C + c0 + e], a[e]);
    }
    Chunk<T>::store(dx + r * C + c0, a);
  }
}

// grid (row slices, n_out): partial[s][o][c] over rows of slice s
template <typename T>
__global__ __launch_bounds__(256) void heads_bwd_dw_partial_kernel(const float* __restrict__ dout,
                                                                   const T* __restrict__ x, int rows, int C,
                                                                   int n_out, int rows_per, float* __restrict__ part,
                                                                   float* __restrict__ partb) {
  const int s = blockIdx.x, o = blockIdx.y;
  const int r0 = s * rows_per, r1 = min(rows, r0 + rows_per);
  __shared__ float scratch[8];
  float bsum = 0.f;
  for (int c = threadIdx.x; c < C; c += 256) {
    float a = 0.f;
    for (int r = r0; r < r1; ++r) a = fmaf(dout[(long)r * n_out + o], (float)x[(long)r * C + c], a);
    part[((long)s * n_out + o) * C + c] = a;
  }
  for (int r = r0 + threadIdx.x; r < r1; r += 256) bsum += dout[(long)r * n_out + o];
  bsum = block_sum<4>(bsum, scratch);
  if (threadIdx.x == 0) partb[(long)s * n_out + o] = bsum;
}

__global__ void heads_bwd_dw_reduce_kernel(const float* __restrict__ part, const float* __restrict__ partb, int S,
                                           int n_out, int C, float* __restrict__ dw, float* __restrict__ db) {
  const long n = (long)n_out * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n + n_out; i += (long)gridDim.x * blockDim.x) {
    float a = 0.f;
    if (i < n) {
      for (int s = 0; s < S; ++s) a += part[(long)s * n + i];
      dw[i] = a;
    } else {
      for (int s = 0; s < S; ++s) a += partb[(long)s * n_out + (i - n)];
      db[i - n] = a;
    }
  }
}

extern "C" long tdeed_heads_bwd_workspace(int rows, int C, int n_out) {
  const int S = rows >= 64 ? 64 : rows;
  return (long)S * n_out * (C + 1) * (long)sizeof(float);
}

extern "C" int tdeed_heads_bwd(const float* dout, const void* x, int rows, int C, const float* w, int n_out,
                               void* dx, float* dw, float* db, void* workspace, int dtype, void* stream) {
  TD_CHECK(dout && x && w && dw && db && workspace, "heads_bwd: null pointer");
  TD_CHECK(rows > 0 && C % 8 == 0 && n_out > 0, "heads_bwd: bad sizes");
  hipStream_t st = (hipStream_t)stream;
  const int S = rows >= 64 ? 64 : rows;
  const int rows_per = (rows + S - 1) / S;
  float* part = (float*)workspace;
  float* partb = part + (long)S * n_out * C;
  if (dtype == TDEED_F32) {
    if (dx) hipLaunchKernelGGL(heads_bwd_dx_kernel<float>, dim3(cdiv((long)rows * (C / 4), 256)), dim3(256), 0, st, dout,
                               rows, C, w, n_out, (float*)dx);
    hipLaunchKernelGGL(heads_bwd_dw_partial_kernel<float>, dim3(S, n_out), dim3(256), 0, st, dout, (const float*)x, rows,
                       C, n_out, rows_per, part, partb);
  } else if (dtype == TDEED_BF16) {
    if (dx) hipLaunchKernelGGL(heads_bwd_dx_kernel<bf16_t>, dim3(cdiv((long)rows * (C / 8), 256)), dim3(256), 0, st, dout,
                               rows, C, w, n_out, (bf16_t*)dx);
    hipLaunchKernelGGL(heads_bwd_dw_partial_kernel<bf16_t>, dim3(S, n_out), dim3(256), 0, st, dout, (const bf16_t*)x,
                       rows, C, n_out, rows_per, part, partb);
  } else { tdeed_set_error("heads_bwd: bad dtype %d", dtype); return TDEED_ERR_ARG; }
  hipLaunchKernelGGL(heads_bwd_dw_reduce_kernel, dim3(cdiv((long)n_out * C + n_out, 256)), dim3(256), 0, st, part, partb,
                     S, n_out, C, dw, db);
  TD_LAUNCH_CHECK("heads_bwd");
  return TDEED_OK;
}

// ------------------------------------------------------------------------------------------ fused AdamW
// torch.optim.AdamW semantics (decoupled decay, bias correction), all tensors fp32, one flat buffer per state:
//   p *= 1 - lr*wd;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;
//   p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// grad_scale multiplies g first (1/world for the data-parallel mean, 1/loss-scale ...).  16-byte vectorised.
// One body for the plain and the guarded kernel (adamw_kernel / adamw_guarded_kernel below).
__device__ __forceinline__ void adamw_update(float* __restrict__ p, const float* __restrict__ g,
                                             float* __restrict__ m, float* __restrict__ v, long n, float lr,
                                             float b1, float b2, float eps, float wd, float bc1, float bc2s,
                                             float gscale) {
  const long n4 = n >> 2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
    const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
    f32x4 mv = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gg = gv[e] * gscale;
      pv[e] *= 1.0f - lr * wd;
      mv[e] = b1 * mv[e] + (1.0f - b1) * gg;
      vv[e] = b2 * vv[e] + (1.0f - b2) * gg * gg;
      pv[e] -= (lr / bc1) * mv[e] / (sqrtf(vv[e]) / bc2s + eps);
    }
    reinterpret_cast<f32x4*>(p)[i] = pv;
    reinterpret_cast<f32x4*>(m)[i] = mv;
    reinterpret_cast<f32x4*>(v)[i] = vv;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long i = (n4 << 2) + threadIdx.x;
    const float gg = g[i] * gscale;
    float pv = p[i] * (1.0f - lr * wd);
    const float mv = b1 * m[i] + (1.0f - b1) * gg;
    const float vv = b2 * v[i] + (1.0f - b2) * gg * gg;
    pv -= (lr / bc1) * mv / (sqrtf(vv) / bc2s + eps);
    p[i] = pv; m[i] = mv; v[i] = vv;
  }
}

__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v, long n, float lr,
                                                    float b1, float b2, float eps, float wd, float bc1, float bc2s,
                                                    float gscale) {
  adamw_update(p, g, m, v, n, lr, b1, b2, eps, wd, bc1, bc2s, gscale);
}

// grid of the flat-buffer kernels: one 16-byte chunk per thread and trip, at most 4096 workgroups of 256
static int flat_grid(long n) {
  const long n4 = n >> 2;
  return (int)(n4 / 256 + 1 < 4096 ? n4 / 256 + 1 : 4096);
}

extern "C" int tdeed_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n,
                                float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                                float grad_scale, void* stream) {
  TD_CHECK(param && grad && exp_avg && exp_avg_sq, "adamw: null pointer");
  TD_CHECK(n > 0 && step >= 1, "adamw: bad n/step");
  TD_CHECK((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0,
           "adamw: buffers must be 16-byte aligned");
  const float bc1 = 1.0f - powf(beta1, (float)step);
  const float bc2s = sqrtf(1.0f - powf(beta2, (float)step));
  hipLaunchKernelGGL(adamw_kernel, dim3(flat_grid(n)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq,
                     n, lr, beta1, beta2, eps, weight_decay, bc1, bc2s, grad_scale);
  TD_LAUNCH_CHECK("adamw");
  return TDEED_OK;
}

// ------------------------------------------------------------------------------------------ guarded AdamW
// What the reference's GradScaler did for the optimizer (modules.py:390-404: scaler.step() leaves the optimizer and its
// step count alone when a gradient holds an inf or a NaN), plus clip_grad_norm_'s rule, without a host synchronisation.
// The statistic both need is the sum of squares of the flat gradient buffer in binary64: the square of an fp32 value is
// exact there and up to 2^31 of them cannot overflow, so the sum is finite exactly when every element is (a buffer of
// FLT_MAX is finite).  Two launches, no atomics, fixed fold order: the bits do not depend on which workgroup runs when.
struct GuardRecord {            // include/tdeed_hip.h: 32 bytes, owned by the caller
  double sumsq;                 // this call, raw buffer (before grad_scale)
  int nonfinite;                // this call, 0 | 1
  int skipped;                  // cumulative: grad_guard_fold_kernel alone writes it
  int reserved[4];
};
static_assert(sizeof(GuardRecord) == 32, "guard record layout");

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// 4 waves; thread 0's return value is the workgroup's sum (waves folded in index order)
__device__ __forceinline__ double block_sum_f64(double v, double* scratch) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((scratch[0] + scratch[1]) + scratch[2]) + scratch[3];
}

// pass one: part[blockIdx.x] = sum of g^2 over the chunks this workgroup walks (+ the scalar tail in workgroup 0)
__global__ __launch_bounds__(256) void grad_guard_partial_kernel(const float* __restrict__ g, long n,
                                                                 double* __restrict__ part) {
  __shared__ double scratch[4];
  const long n4 = n >> 2;
  double acc = 0.0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = fma((double)gv[e], (double)gv[e], acc);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const double t = (double)g[(n4 << 2) + threadIdx.x];
    acc = fma(t, t, acc);
  }
  acc = block_sum_f64(acc, scratch);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// pass two: one workgroup; thread t takes partials t, t + 256, ... in index order, then the same fixed fold
__global__ __launch_bounds__(256) void grad_guard_fold_kernel(const double* __restrict__ part, int nparts,
                                                              int skip_nonfinite, GuardRecord* __restrict__ rec) {
  __shared__ double scratch[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) acc += part[i];
  acc = block_sum_f64(acc, scratch);
  if (threadIdx.x == 0) {
    const int bad = __builtin_isfinite(acc) ? 0 : 1;
    const int skipped = rec->skipped + (skip_nonfinite ? bad : 0);
    rec->sumsq = acc;
    rec->nonfinite = bad;
    rec->skipped = skipped;
#pragma unroll
    for (int e = 0; e < 4; ++e) rec->reserved[e] = 0;
  }
}

extern "C" long tdeed_grad_guard_ws_bytes(long n) { return n > 0 ? (long)flat_grid(n) * (long)sizeof(double) : 0; }

extern "C" int tdeed_grad_guard(const float* grad, long n, int skip_nonfinite, void* guard, void* ws, void* stream) {
  TD_CHECK(grad && guard && ws, "grad_guard: null pointer");
  TD_CHECK(n > 0, "grad_guard: bad n");
  TD_CHECK((((uintptr_t)grad | (uintptr_t)guard) & 15) == 0 && ((uintptr_t)ws & 7) == 0,
           "grad_guard: grad and the record must be 16-byte aligned, the workspace 8-byte aligned");
  const int grid = flat_grid(n);
  hipLaunchKernelGGL(grad_guard_partial_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, grad, n, (double*)ws);
  hipLaunchKernelGGL(grad_guard_fold_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)ws, grid,
                     skip_nonfinite, (GuardRecord*)guard);
  TD_LAUNCH_CHECK("grad_guard");
  return TDEED_OK;
}

// adamw_update behind the record (every thread reads it once; the addresses are uniform).  bc1 / bc2s are the host's, for
// the host's count of attempts `step`: they are used as they are while nothing was skipped, so that on finite gradients
// without clipping this launch writes the bits adamw_kernel writes.  After a skip the effective step is step - skipped and
// the corrections come from the device's powf (a few ulp from glibc's).
__global__ __launch_bounds__(256) void adamw_guarded_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                            float* __restrict__ m, float* __restrict__ v, long n, float lr,
                                                            float b1, float b2, float eps, float wd, float bc1, float bc2s,
                                                            float gscale, int step, const GuardRecord* __restrict__ rec,
                                                            int skip_nonfinite, float max_norm) {
  const double sumsq = rec->sumsq;
  const int nonfinite = rec->nonfinite, skipped = rec->skipped;
  if (skip_nonfinite && nonfinite) return;
  if (max_norm > 0.0f) {
    // clip_grad_norm_: coef = clamp(max_norm / (norm + 1e-6), max=1), the norm being that of the gradient AdamW sees.
    // A NaN norm gives a NaN coefficient (torch's clamp keeps it), an infinite one 0: not special-cased.
    const float norm = (float)((double)gscale * sqrt(sumsq));
    const float q = max_norm / (norm + 1e-6f);
    gscale *= q > 1.0f ? 1.0f : q;
  }
  if (skipped != 0) {
    const float t = (float)(step - skipped);
    bc1 = 1.0f - powf(b1, t);
    bc2s = sqrtf(1.0f - powf(b2, t));
  }
  adamw_update(p, g, m, v, n, lr, b1, b2, eps, wd, bc1, bc2s, gscale);
}

extern "C" int tdeed_adamw_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n,
                                        float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                                        float grad_scale, const void* guard, int skip_nonfinite, float max_grad_norm,
                                        void* stream) {
  TD_CHECK(param && grad && exp_avg && exp_avg_sq && guard, "adamw_guarded: null pointer");
  TD_CHECK(n > 0 && step >= 1, "adamw_guarded: bad n/step");
  TD_CHECK((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)guard) & 15) == 0,
           "adamw_guarded: buffers and the record must be 16-byte aligned");
  const float bc1 = 1.0f - powf(beta1, (float)step);
  const float bc2s = sqrtf(1.0f - powf(beta2, (float)step));
  hipLaunchKernelGGL(adamw_guarded_kernel, dim3(flat_grid(n)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                     exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2s, grad_scale, step,
                     (const GuardRecord*)guard, skip_nonfinite, max_grad_norm);
  TD_LAUNCH_CHECK("adamw_guarded");
  return TDEED_OK;
}

// ------------------------------------------------------------------------------------------ AdamW over runs
// Parameter groups (optim.group_table): the flat buffer is a sequence of runs, each with its own lr scale and weight decay,
// or frozen.  One record per run, written by the host once (FusedAdamW.set_groups); every run boundary is a multiple of 4
// elements, so a 16-byte chunk lies in exactly one run.  The run ends are staged in LDS; a thread finds its chunk's run by
// bisection from the run of its previous trip (neighbouring lanes read the same words: broadcasts), then the arithmetic is
// adamw_update's (adamw_element below) with lr * lr_scale (one fp32 product) and the run's decay.  A frozen run loads and
// stores nothing.  The table's content cannot move an access: i < n4 bounds the buffers, nruns the table.
struct AdamwRun {               // include/tdeed_hip.h: 16 bytes
  int end4;                     // end of the run in 16-byte chunks (exclusive); the last run's covers ceil(n / 4)
  float lr_scale;
  float wd;                     // < 0: the launch's weight_decay
  int frozen;
};
static_assert(sizeof(AdamwRun) == 16, "run record layout");
#define ADAMW_MAX_RUNS 16384    // 64 KiB of run ends in LDS

// adamw_update's element arithmetic with the roundings spelled out.  Under -ffp-contract=fast the compiler chooses which
// products of adamw_update fuse into an fma, and it chooses differently once lr and wd vary per thread.  Bit identity with
// adamw_kernel / adamw_guarded_kernel therefore cannot be left to it: contraction is off in here and the fmas below are the
// ones those two kernels compile to on gfx950 -- in the 16-byte loop (TAIL = false) decay = fma(-lr, wd, 1),
// m = fma(1 - b1, gg, b1 m), v = fma(b2, v, gg ((1 - b2) gg)), p = fma(decay, p, -q); in the scalar tail (TAIL = true) v and
// p are a product and a separate sum.  tests/test_gpu_param_groups.py holds every run to the plain launch bit for bit, so
// a compiler that contracts adamw_update differently shows up there.
template <bool TAIL>
__device__ __forceinline__ void adamw_element(float& pv, float& mv, float& vv, float g, float lr, float b1, float b2,
                                              float eps, float wd, float bc1, float bc2s, float gscale) {
#pragma clang fp contract(off)
  const float gg = g * gscale;
  const float decay = __builtin_fmaf(-lr, wd, 1.0f);
  mv = __builtin_fmaf(1.0f - b1, gg, b1 * mv);
  const float g2 = gg * ((1.0f - b2) * gg);
  vv = TAIL ? g2 + b2 * vv : __builtin_fmaf(b2, vv, g2);
  const float q = ((lr / bc1) * mv) / (sqrtf(vv) / bc2s + eps);
  pv = TAIL ? decay * pv - q : __builtin_fmaf(decay, pv, -q);
}

template <bool GUARDED>
__global__ __launch_bounds__(256) void adamw_groups_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v, long n, float lr,
                                                           float b1, float b2, float eps, float wd, float bc1, float bc2s,
                                                           float gscale, int step, const GuardRecord* __restrict__ rec,
                                                           int skip_nonfinite, float max_norm,
                                                           const AdamwRun* __restrict__ runs, int nruns) {
  extern __shared__ int run_end[];
  if (GUARDED) {                // adamw_guarded_kernel's prologue; the early return is uniform over the grid
    const double sumsq = rec->sumsq;
    const int nonfinite = rec->nonfinite, skipped = rec->skipped;
    if (skip_nonfinite && nonfinite) return;
    if (max_norm > 0.0f) {
      const float norm = (float)((double)gscale * sqrt(sumsq));
      const float q = max_norm / (norm + 1e-6f);
      gscale *= q > 1.0f ? 1.0f : q;
    }
    if (skipped != 0) {
      const float t = (float)(step - skipped);
      bc1 = 1.0f - powf(b1, t);
      bc2s = sqrtf(1.0f - powf(b2, t));
    }
  }
  for (int r = threadIdx.x; r < nruns; r += 256) run_end[r] = runs[r].end4;
  __syncthreads();
  const long n4 = n >> 2;
  int r = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    if ((long)run_end[r] <= i) {                                 // first run in (r, nruns - 1] that ends behind chunk i
      int lo = r + 1, hi = nruns - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long)run_end[mid] > i) hi = mid; else lo = mid + 1;
      }
      r = lo < nruns ? lo : nruns - 1;
    }
    const AdamwRun run = runs[r];
    if (run.frozen) continue;
    const float lr_s = lr * run.lr_scale, wd_s = run.wd < 0.0f ? wd : run.wd;
    f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
    const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
    f32x4 mv = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float pe = pv[e], me = mv[e], ve = vv[e];
      adamw_element<false>(pe, me, ve, gv[e], lr_s, b1, b2, eps, wd_s, bc1, bc2s, gscale);
      pv[e] = pe; mv[e] = me; vv[e] = ve;
    }
    reinterpret_cast<f32x4*>(p)[i] = pv;
    reinterpret_cast<f32x4*>(m)[i] = mv;
    reinterpret_cast<f32x4*>(v)[i] = vv;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {                // the scalar tail belongs to the last run
    const AdamwRun run = runs[nruns - 1];
    if (run.frozen) return;
    const float lr_s = lr * run.lr_scale, wd_s = run.wd < 0.0f ? wd : run.wd;
    const long i = (n4 << 2) + threadIdx.x;
    float pe = p[i], me = m[i], ve = v[i];
    adamw_element<true>(pe, me, ve, g[i], lr_s, b1, b2, eps, wd_s, bc1, bc2s, gscale);
    p[i] = pe; m[i] = me; v[i] = ve;
  }
}

extern "C" int tdeed_adamw_step_groups(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n,
                                       float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                                       float grad_scale, const void* guard, int skip_nonfinite, float max_grad_norm,
                                       const void* runs, int nruns, void* stream) {
  TD_CHECK(param && grad && exp_avg && exp_avg_sq && runs, "adamw_groups: null pointer");
  TD_CHECK(n > 0 && step >= 1, "adamw_groups: bad n/step");
  TD_CHECK((n >> 2) < 0x7fffffffL, "adamw_groups: the run table counts 16-byte chunks in 31 bits");
  TD_CHECK(nruns >= 1 && nruns <= ADAMW_MAX_RUNS, "adamw_groups: 1 .. 16384 runs");
  TD_CHECK((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)guard |
             (uintptr_t)runs) & 15) == 0, "adamw_groups: buffers, the record and the run table must be 16-byte aligned");
  const float bc1 = 1.0f - powf(beta1, (float)step);
  const float bc2s = sqrtf(1.0f - powf(beta2, (float)step));
  const size_t lds = (size_t)nruns * sizeof(int);
  if (guard)
    hipLaunchKernelGGL(adamw_groups_kernel<true>, dim3(flat_grid(n)), dim3(256), lds, (hipStream_t)stream, param, grad,
                       exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2s, grad_scale, step,
                       (const GuardRecord*)guard, skip_nonfinite, max_grad_norm, (const AdamwRun*)runs, nruns);
  else
    hipLaunchKernelGGL(adamw_groups_kernel<false>, dim3(flat_grid(n)), dim3(256), lds, (hipStream_t)stream, param, grad,
                       exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2s, grad_scale, step,
                       (const GuardRecord*)nullptr, 0, 0.0f, (const AdamwRun*)runs, nruns);
  TD_LAUNCH_CHECK("adamw_groups");
  return TDEED_OK;
}

// ------------------------------------------------------------------------------------------ AdamW + weight EMA
// An exponential moving average of the weights (the shadow `ema`, one more flat fp32 buffer), updated in the launch that
// writes the new parameter: e += w (p_new - e) on the value still in registers, so the shadow costs one load and one store
// per element and no second read of p.  All fp32, nothing fused, three roundings (diff, prod, sum).
//   n   = (step - skipped) - ema_step0      applied updates since the shadow was switched on, this one included (>= 1)
//   d_n = warmup ? min(d, (1 + n) / (10 + n)) : d;   w = 1 - d_n
// The quotient is a binary64 division rounded to fp32: for operands below 2^24 that is the correctly rounded fp32 quotient
// (53 >= 2 * 24 + 2 bits), whatever the flags make of an fp32 division.  optim.ema_ref restates this on the host.
__device__ __forceinline__ float ema_weight(int n, float d, int warmup) {
  if (n < 1) n = 1;                                             // (the entry checks step - ema_step0 >= 1)
  float dn = d;
  if (warmup) {
    const float q = (float)((double)(1 + n) / (double)(10 + n));
    dn = q < d ? q : d;
  }
  return 1.0f - dn;
}

// -ffp-contract=fast lets the backend fuse the product into the sum whatever a pragma says (it did: v_fmac_f32), so the
// product passes through an empty asm statement: the compiler must materialise it, rounded, before the sum.
__device__ __forceinline__ float ema_element(float e, float p_new, float w) {
  const float diff = p_new - e;
  float prod = w * diff;
  asm("" : "+v"(prod));
  return e + prod;
}

// adamw_groups_kernel's body (adamw_element; GROUPS = false is one neutral run: lr * 1 and the launch's decay, the bits of
// adamw_kernel / adamw_guarded_kernel) with the shadow update behind it.  A skipped step returns before anything is read; a
// frozen run neither loads nor stores its shadow slice (it equals the parameters from the moment EMA was switched on).
template <bool GUARDED, bool GROUPS>
__global__ __launch_bounds__(256) void adamw_ema_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v,
                                                        float* __restrict__ ema, long n, float lr, float b1, float b2,
                                                        float eps, float wd, float bc1, float bc2s, float gscale, int step,
                                                        const GuardRecord* __restrict__ rec, int skip_nonfinite,
                                                        float max_norm, const AdamwRun* __restrict__ runs, int nruns,
                                                        float ema_decay, int ema_warmup, int ema_step0) {
  extern __shared__ int run_end[];
  int skipped = 0;
  if (GUARDED) {                // adamw_guarded_kernel's prologue; the early return is uniform over the grid
    const double sumsq = rec->sumsq;
    const int nonfinite = rec->nonfinite;
    skipped = rec->skipped;
    if (skip_nonfinite && nonfinite) return;
    if (max_norm > 0.0f) {
      const float norm = (float)((double)gscale * sqrt(sumsq));
      const float q = max_norm / (norm + 1e-6f);
      gscale *= q > 1.0f ? 1.0f : q;
    }
    if (skipped != 0) {
      const float t = (float)(step - skipped);
      bc1 = 1.0f - powf(b1, t);
      bc2s = sqrtf(1.0f - powf(b2, t));
    }
  }
  const float ew = ema_weight(step - skipped - ema_step0, ema_decay, ema_warmup);
  if (GROUPS) {
    for (int r = threadIdx.x; r < nruns; r += 256) run_end[r] = runs[r].end4;
    __syncthreads();
  }
  const long n4 = n >> 2;
  int r = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    float lr_s = lr, wd_s = wd;
    if (GROUPS) {
      if ((long)run_end[r] <= i) {                               // first run in (r, nruns - 1] that ends behind chunk i
        int lo = r + 1, hi = nruns - 1;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if ((long)run_end[mid] > i) hi = mid; else lo = mid + 1;
        }
        r = lo < nruns ? lo : nruns - 1;
      }
      const AdamwRun run = runs[r];
      if (run.frozen) continue;
      lr_s = lr * run.lr_scale;
      wd_s = run.wd < 0.0f ? wd : run.wd;
    }
    f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
    const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
    f32x4 mv = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
    f32x4 ev = reinterpret_cast<f32x4*>(ema)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float pe = pv[e], me = mv[e], ve = vv[e];
      adamw_element<false>(pe, me, ve, gv[e], lr_s, b1, b2, eps, wd_s, bc1, bc2s, gscale);
      pv[e] = pe; mv[e] = me; vv[e] = ve;
      ev[e] = ema_element(ev[e], pe, ew);
    }
    reinterpret_cast<f32x4*>(p)[i] = pv;
    reinterpret_cast<f32x4*>(m)[i] = mv;
    reinterpret_cast<f32x4*>(v)[i] = vv;
    reinterpret_cast<f32x4*>(ema)[i] = ev;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {                // the scalar tail belongs to the last run
    float lr_s = lr, wd_s = wd;
    if (GROUPS) {
      const AdamwRun run = runs[nruns - 1];
      if (run.frozen) return;
      lr_s = lr * run.lr_scale;
      wd_s = run.wd < 0.0f ? wd : run.wd;
    }
    const long i = (n4 << 2) + threadIdx.x;
    float pe = p[i], me = m[i], ve = v[i];
    adamw_element<true>(pe, me, ve, g[i], lr_s, b1, b2, eps, wd_s, bc1, bc2s, gscale);
    p[i] = pe; m[i] = me; v[i] = ve;
    ema[i] = ema_element(ema[i], pe, ew);
  }
}

template <bool GUARDED, bool GROUPS>
static void launch_adamw_ema(int grid, size_t lds, hipStream_t stream, float* p, const float* g, float* m, float* v,
                             float* ema, long n, float lr, float b1, float b2, float eps, float wd, float bc1, float bc2s,
                             float gscale, int step, const GuardRecord* rec, int skip_nonfinite, float max_norm,
                             const AdamwRun* runs, int nruns, float ema_decay, int ema_warmup, int ema_step0) {
  hipLaunchKernelGGL((adamw_ema_kernel<GUARDED, GROUPS>), dim3(grid), dim3(256), lds, stream, p, g, m, v, ema, n, lr, b1, b2,
                     eps, wd, bc1, bc2s, gscale, step, rec, skip_nonfinite, max_norm, runs, nruns, ema_decay, ema_warmup,
                     ema_step0);
}

extern "C" int tdeed_adamw_step_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, float lr,
                                    float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                                    const void* guard, int skip_nonfinite, float max_grad_norm, const void* runs, int nruns,
                                    float* ema, float ema_decay, int ema_warmup, int ema_step0, void* stream) {
  TD_CHECK(param && grad && exp_avg && exp_avg_sq && ema, "adamw_ema: null pointer");
  TD_CHECK(n > 0 && step >= 1, "adamw_ema: bad n/step");
  TD_CHECK((n >> 2) < 0x7fffffffL, "adamw_ema: the run table counts 16-byte chunks in 31 bits");
  TD_CHECK(!runs || (nruns >= 1 && nruns <= ADAMW_MAX_RUNS), "adamw_ema: 1 .. 16384 runs");
  TD_CHECK((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)guard |
             (uintptr_t)runs | (uintptr_t)ema) & 15) == 0,
           "adamw_ema: buffers, the shadow, the record and the run table must be 16-byte aligned");
  TD_CHECK(ema_decay > 0.0f && ema_decay < 1.0f, "adamw_ema: 0 < ema_decay < 1");
  TD_CHECK(ema_step0 >= 0 && step - ema_step0 >= 1, "adamw_ema: ema_step0 >= 0 and step - ema_step0 >= 1");
  const float bc1 = 1.0f - powf(beta1, (float)step);
  const float bc2s = sqrtf(1.0f - powf(beta2, (float)step));
  const size_t lds = runs ? (size_t)nruns * sizeof(int) : 0;
  const int grid = flat_grid(n);
  const GuardRecord* rec = (const GuardRecord*)guard;
  if (!guard) { skip_nonfinite = 0; max_grad_norm = 0.0f; }
  if (!runs) nruns = 0;
#define TD_EMA_LAUNCH(G, R)                                                                                              \
  launch_adamw_ema<G, R>(grid, lds, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, ema, n, lr, beta1, beta2, eps, \
                         weight_decay, bc1, bc2s, grad_scale, step, rec, skip_nonfinite, max_grad_norm,                  \
                         (const AdamwRun*)runs, nruns, ema_decay, ema_warmup ? 1 : 0, ema_step0)
  if (guard && runs) TD_EMA_LAUNCH(true, true);
  else if (guard) TD_EMA_LAUNCH(true, false);
  else if (runs) TD_EMA_LAUNCH(false, true);
  else TD_EMA_LAUNCH(false, false);
#undef TD_EMA_LAUNCH
  TD_LAUNCH_CHECK("adamw_ema");
  return TDEED_OK;
}

// The same average for tensors outside the flat buffer (the BatchNorm running statistics): a device table of 16-byte rows,
// written by the host once and uploaded once; one workgroup per row, lanes stride over the row.  `host_rows` is the host's
// copy of the table: the entry checks every row against the shadow's length before the launch, and the kernel bounds each
// row by shadow_n again, so the table's content cannot move a store outside the shadow.
struct EmaRow {                 // include/tdeed_hip.h: 16 bytes
  const float* src;
  int offset;                   // first element of the row in the shadow
  int count;
};
static_assert(sizeof(EmaRow) == 16, "ema row layout");
#define EMA_MAX_ROWS 65535

__global__ __launch_bounds__(256) void ema_tensors_kernel(const EmaRow* __restrict__ rows, float* __restrict__ shadow,
                                                          long shadow_n, int step, const GuardRecord* __restrict__ rec,
                                                          int skip_nonfinite, float ema_decay, int ema_warmup,
                                                          int ema_step0) {
  int skipped = 0;
  if (rec) {                    // uniform over the grid
    skipped = rec->skipped;
    if (skip_nonfinite && rec->nonfinite) return;
  }
  const float ew = ema_weight(step - skipped - ema_step0, ema_decay, ema_warmup);
  const EmaRow row = rows[blockIdx.x];
  if (row.offset < 0 || row.count < 0 || (long)row.offset + row.count > shadow_n) return;
  float* __restrict__ dst = shadow + row.offset;
  for (int i = threadIdx.x; i < row.count; i += 256) dst[i] = ema_element(dst[i], row.src[i], ew);
}

extern "C" int tdeed_ema_tensors(const void* rows, const void* host_rows, int nrows, float* shadow, long shadow_n, int step,
                                 const void* guard, int skip_nonfinite, float ema_decay, int ema_warmup, int ema_step0,
                                 void* stream) {
  TD_CHECK(rows && host_rows && shadow, "ema_tensors: null pointer");
  TD_CHECK(nrows >= 1 && nrows <= EMA_MAX_ROWS, "ema_tensors: 1 .. 65535 rows");
  TD_CHECK(shadow_n > 0 && step >= 1, "ema_tensors: bad shadow length / step");
  TD_CHECK((((uintptr_t)rows | (uintptr_t)guard) & 15) == 0 && ((uintptr_t)shadow & 3) == 0,
           "ema_tensors: the table and the record must be 16-byte aligned, the shadow 4-byte aligned");
  TD_CHECK(ema_decay > 0.0f && ema_decay < 1.0f, "ema_tensors: 0 < ema_decay < 1");
  TD_CHECK(ema_step0 >= 0 && step - ema_step0 >= 1, "ema_tensors: ema_step0 >= 0 and step - ema_step0 >= 1");
  const EmaRow* hr = (const EmaRow*)host_rows;
  for (int r = 0; r < nrows; ++r) {
    TD_CHECK(hr[r].src && ((uintptr_t)hr[r].src & 3) == 0, "ema_tensors: row %d: null or misaligned source", r);
    TD_CHECK(hr[r].offset >= 0 && hr[r].count >= 1 && (long)hr[r].offset + hr[r].count <= shadow_n,
             "ema_tensors: row %d (offset %d, count %d) overruns the shadow of %ld elements", r, hr[r].offset, hr[r].count,
             shadow_n);
  }
  hipLaunchKernelGGL(ema_tensors_kernel, dim3(nrows), dim3(256), 0, (hipStream_t)stream, (const EmaRow*)rows, shadow,
                     shadow_n, step, (const GuardRecord*)guard, guard ? skip_nonfinite : 0, ema_decay, ema_warmup ? 1 : 0,
                     ema_step0);
  TD_LAUNCH_CHECK("ema_tensors");
  return TDEED_OK;
}

// =========================================================================== joint-dataset (double head) loss
// model.py:278-306: the class head is two heads side by side (K1a | K1b columns); clip i belongs to dataset ds[i] in
// {1, 2} and is scored on its own slice only: loss = sum_i CE_i / B with CE_i = sum_t w[y] nll / sum_t w[y] over the
// clip's T frames (labels of dataset 2 arrive shifted by K1a: update_labels_2heads), + the displacement MSE over all rows.
// One workgroup walks the clips (B is a few dozen, T a few hundred): fixed-order sums.
__global__ __launch_bounds__(256) void loss2_kernel(const float* __restrict__ head, int B, int T_len, int ld, int K1a,
                                                    int K1b, const int64_t* __restrict__ ds,
                                                    const int64_t* __restrict__ hard, const float* __restrict__ soft,
                                                    const float* __restrict__ cls_w,
                                                    int displ_col, const float* __restrict__ labelD, float gscale,
                                                    float* __restrict__ out, float* __restrict__ dhead) {
  __shared__ float scratch[8];
  float ce = 0.f, se_tot = 0.f, bad = 0.f;
  const long rows = (long)B * T_len;
  const int Ks = K1a + K1b;                                       // soft rows: distributions over both heads' columns
  for (int i = 0; i < B; ++i) {
    const bool first = ds[i] == 1;
    const int col0 = first ? 0 : K1a, K = first ? K1a : K1b;
    float num = 0.f, den = 0.f, se = 0.f;
    for (int t = threadIdx.x; t < T_len; t += 256) {
      const long r = (long)i * T_len + t;
      const float* lg = head + r * ld + col0;
      float m = lg[0];
      for (int k = 1; k < K; ++k) m = fmaxf(m, lg[k]);
      float s = 0.f;
      for (int k = 0; k < K; ++k) s += expf(lg[k] - m);
      const float lse = m + logf(s);
      if (soft) {                                                 // mixup: -sum_c w_c p_c log softmax_c, mean over the T rows
        const float* p = soft + r * Ks + col0;
        for (int k = 0; k < K; ++k) num += cls_w[k] * p[k] * (lse - lg[k]);
      } else {
        int y = (int)hard[r] - col0;
        if (y < 0 || y >= K) { bad = 1.f; y = 0; }              // label outside the clip's own head: never indexed, loss -> NaN
        const float w = cls_w[y];
        num += w * (lse - lg[y]);
        den += w;
      }
      if (displ_col >= 0 && labelD) {
        const float d = head[r * ld + displ_col] - labelD[r];
        se += d * d;
      }
    }
    num = block_sum<4>(num, scratch);
    den = soft ? (float)T_len : block_sum<4>(den, scratch);
    se = block_sum<4>(se, scratch);
    ce += num / den / (float)B;
    se_tot += se;
    if (dhead) {
      const float inv = gscale / (den * (float)B);
      for (int t = threadIdx.x; t < T_len; t += 256) {
        const long r = (long)i * T_len + t;
        const float* lg = head + r * ld + col0;
        float* dg = dhead + r * ld;
        for (int k = 0; k < ld; ++k) dg[k] = 0.f;
        float m = lg[0];
        for (int k = 1; k < K; ++k) m = fmaxf(m, lg[k]);
        float s = 0.f;
        for (int k = 0; k < K; ++k) s += expf(lg[k] - m);
        const float is = 1.0f / s;
        if (soft) {
          const float* p = soft + r * Ks + col0;
          float wp = 0.f;
          for (int k = 0; k < K; ++k) wp += cls_w[k] * p[k];
          for (int k = 0; k < K; ++k) dg[col0 + k] = (expf(lg[k] - m) * is * wp - cls_w[k] * p[k]) * inv;
        } else {
          int y = (int)hard[r] - col0;
          if (y < 0 || y >= K) y = 0;
          const float wy = cls_w[y];
          for (int k = 0; k < K; ++k) dg[col0 + k] = wy * (expf(lg[k] - m) * is - (k == y ? 1.f : 0.f)) * inv;
        }
        if (displ_col >= 0 && labelD) dg[displ_col] = 2.0f * (head[r * ld + displ_col] - labelD[r]) * gscale / (float)rows;
      }
    }
  }
  bad = block_sum<4>(bad, scratch);
  if (threadIdx.x == 0 && out) {
    const float mse = (displ_col >= 0 && labelD) ? se_tot / (float)rows : 0.f;
    if (bad > 0.f) ce = __builtin_nanf("");                     // torch's cross_entropy raises here; a NaN loss is this path's alarm
    out[0] = ce + mse;
    out[1] = ce;
    out[2] = mse;
  }
}

// out fp32 [3] (total, CE, MSE) and/or dhead fp32 [B*T][ld] (either may be NULL); cls_w has max(K1a, K1b) entries.
// hard: int64 [B*T] labels over the concatenated heads, or soft: fp32 [B*T][K1a+K1b] (mixup; model.py:278-306 with 3-D labels).
// A hard label outside its clip's head slice is never used as an index: the row gets class 0 and the loss becomes NaN.
extern "C" int tdeed_loss2(const float* head_out, int B, int T, int ld, int K1a, int K1b, const int64_t* dataset,
                           const int64_t* hard, const float* soft, const float* cls_w, int displ_col, const float* labelD,
                           float grad_scale, float* out, float* dhead, void* stream) {
  TD_CHECK(head_out && dataset && (hard || soft) && cls_w && (out || dhead), "loss2: null pointer");
  TD_CHECK(B > 0 && T > 0 && K1a > 0 && K1b > 0 && K1a + K1b <= ld && displ_col < ld, "loss2: bad sizes");
  hipLaunchKernelGGL(loss2_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, head_out, B, T, ld, K1a, K1b, dataset, hard,
                     soft, cls_w, displ_col, labelD, grad_scale, out, dhead);
  TD_LAUNCH_CHECK("loss2");
  return TDEED_OK;
}
