/* tdeed_hip.h -- C ABI of libtdeed_hip.so, the gfx950 (MI355X) kernels of the T-DEED hot path.
 *
 * The reference (arturxe2/T-DEED) has no FFI/plugin layer: its "operator interface" for this
 * path is the set of torch.nn module calls inside TDEEDModel.Impl.forward
 * (/root/reference/model/model.py:105-149) and the loss in TDEEDModel.epoch (model.py:308-319).
 * Each entry point below replaces one fused group of those calls; the cited file:line is what
 * it replaces.  Conventions:
 *   - plain pointers + sizes; every pointer is DEVICE memory owned by the caller (hipMalloc /
 *     torch tensor .data_ptr()); the library allocates nothing and never synchronises;
 *   - `stream` is a hipStream_t passed as void*; all work is stream-ordered on it;
 *   - `dtype` selects the storage type of activations and dense weights: TDEED_F32 (parity
 *     mode, exact-f32 MFMA / VALU) or TDEED_BF16 (throughput mode, fp32 accumulation);
 *     parameters documented as `float*` are always fp32;
 *   - activations are channels-last: images NHWC ([frame][y][x][c]), sequences NTC ([clip][t][c]);
 *   - return 0 on success, <0 on error; tdeed_last_error() gives the message (thread-local).
 * Channel counts must be multiples of 8 (true for every RegNetY-200MF/800MF and SGP width).
 */
#ifndef TDEED_HIP_H
#define TDEED_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { TDEED_F32 = 0, TDEED_BF16 = 1 };
enum { TDEED_ACT_NONE = 0, TDEED_ACT_RELU = 1, TDEED_ACT_GELU = 2 };
enum { TDEED_OK = 0, TDEED_ERR_ARG = -1, TDEED_ERR_LAUNCH = -2, TDEED_ERR_RUNTIME = -3 };

const char* tdeed_last_error(void);
int tdeed_abi_version(void);
/* Device sanity: returns 0 and fills name (<=63 chars) / CU count when device `dev` is gfx950. */
int tdeed_device_info(int dev, char* name64, int* n_cu, int* is_gfx950);

/* ---- pre-proc + stem -------------------------------------------------------------------
 * normalize /255, crop, optional h-flip, ImageNet standardize (model.py:107-129,151-167) fused
 * into timm RegNet stem Conv3x3 s2 (3->32) + BN(eval, folded to scale/shift) + ReLU (model.py:133).
 * frames: uint8 [N][3][H][W] (NCHW as the loader delivers it); out: [N][Ho][Wo][32], Ho=(crop_h+1)/2. */
int tdeed_stem_fwd(const void* frames /* uint8, or fp32 0..255 when frames_f32 (mixup batches) */, int frames_f32,
                   int N, int H, int W, int crop_top, int crop_left,
                   int crop_h, int crop_w, int flip /* all frames (eval TTA, model.py:159-162) */,
                   const unsigned char* flip_mask /* NULL, or [N] per-frame h-flip flags: the train-time
                                                     RandomHorizontalFlip drawn per clip (model.py:83,154-157) */,
                   const float* w /*[32][3][3][3]*/,
                   const float* scale /*[32]*/, const float* shift /*[32]*/, void* out,
                   int relu /* 0: raw conv*scale+shift (training) */, int dtype, void* stream);

/* Training stem (bf16): the same pre-processing + conv on the MFMA pipe, RAW conv output z [N][Ho][Wo][32] (BatchNorm runs
 * on batch statistics in training, model.py:133 under .train()) and per workgroup the per-channel sum / sum of squares of what
 * it stored: colpart fp32 [N * tdeed_stem_mfma_parts(crop_h, crop_w)][2][32] (fold with tdeed_bn_finalize(colpart,
 * colpart + 32, 64, N * parts, N*Ho*Wo, 32, ...)).  wfrag: the [2][2][64][8] fragments of tdeed_s1_front_fwd's stem_wf in fp32 (operands are split into bf16 head + tail
 * in the kernel: three MFMAs per product, z is the fp32 conv rounded once).
 * frames / crop / flip / flip_mask as tdeed_stem_fwd.  tdeed_stem_mfma_parts == 0: the row band does not fit LDS. */
int tdeed_stem_mfma_parts(int crop_h, int crop_w);
int tdeed_stem_mfma_fwd(const void* frames, int frames_f32, int N, int H, int W, int crop_top, int crop_left, int crop_h,
                        int crop_w, int flip, const unsigned char* flip_mask, const void* wfrag, void* z, float* colpart,
                        void* stream);
/* The eval instance of the same kernel body (a frozen, eval-mode stem inside the training step): the folded BatchNorm and
 * the ReLU on the fp32 accumulator, out [N][Hs][Ws][32] bf16 = relu(scale[c] * conv + shift[c]) with ONE rounding; no column
 * sums.  scale / shift: fp32 [32], 16-byte aligned.  Served geometries: tdeed_stem_mfma_parts(crop_h, crop_w) > 0. */
int tdeed_stem_mfma_eval_fwd(const void* frames, int frames_f32, int N, int H, int W, int crop_top, int crop_left, int crop_h,
                             int crop_w, int flip, const unsigned char* flip_mask, const void* wfrag, const float* scale,
                             const float* shift, void* out, void* stream);

/* ---- fused trunk front (bf16 only): pre-proc + stem + s1.b1.conv1 + s1.b1.conv2 (+SE squeeze) + s1.b1.downsample
 * uint8 frames [N][3][H][W] -> y2 [N][Ho][Wo][C1] (conv2 output), shortcut [N][Ho][Wo][C1], pooled fp32
 * [N][parts][C1] partial sums of y2 (parts = tdeed_s1_front_parts(crop_h, crop_w, C1)).  The 112^2 stem and conv1
 * maps stay in LDS / MFMA accumulators (front.hip: a workgroup walks a strip of output rows over rings of input and
 * conv1 rows; parts = strips per frame, a function of the shape and of TDEED_FRONT_ROLL / TDEED_FRONT_PIPE only, never of
 * the frames' alignment).  Weight fragments are pre-packed by
 * tdeed_amd.packing.pack_front_weights; scale/shift are the folded eval BatchNorms (fp32). */
int tdeed_s1_front_parts(int crop_h, int crop_w, int C1);
int tdeed_s1_front_fwd(const uint8_t* frames, int N, int H, int W, int crop_top, int crop_left, int crop_h,
                       int crop_w, int flip, const void* stem_wf, const float* stem_sc, const float* stem_sh,
                       int C1, const void* w1f, const float* sc1, const float* sh1, const void* wdf,
                       const float* scd, const float* shd, const void* w2f, const float* sc2,
                       const float* sh2, void* y2, void* shortcut, float* pooled, void* stream);

/* ---- dense 1x1 contraction (MFMA) ---------------------------------------------------------
 * C[m][n] = act( (sum_k A'[m][k] * W[n][k]) * scale[n] + shift[n] + R[m][n] )
 * Replaces every 1x1 Conv2d+BN(eval)(+ReLU) of the RegNetY trunk incl. the stride-2 shortcut,
 * the SE re-scale in front of conv3, the residual add + ReLU (timm Bottleneck, model.py:133),
 * GatedShift's channel splice (shift.py:89-93) and the SGP mlp / concat_fc Conv1d(k=1)
 * (modules.py:134-138,186,248-254,308-309,316).
 *   A   [M][K] row stride lda (elements).  If A0 != NULL, columns [0,k0) are read from A0
 *       (row stride lda0) instead: the gate-shift output spliced in front of the pass-through
 *       channels.  If a_scale != NULL: A'[m][k] = A[m][k] * a_scale[(m / a_scale_rows)*K + k]
 *       (SE gate per frame).  If gather_stride > 1: row m = (f, yo, xo) of an
 *       [F][gather_ho][gather_wo] grid reads input row (f, yo*s, xo*s) of [F][gather_hi][gather_wi].
 *   W   [N][K] row stride ldw, same dtype as A.   scale/shift: fp32 [N], either may be NULL.
 *   R   optional residual [M][N] row stride ldr.   C: [M][N] row stride ldc.
 * K, N, k0, lda, lda0, ldw, ldr, ldc must be multiples of 8.
 *   colpart  optional fp32 [ceil(M/128)][2][N]: per 128-row tile the column sums and sums of squares of the stored C
 *       (training: the BatchNorm batch statistics of a raw conv output come out of the conv's own epilogue; fold them
 *       with tdeed_bn_finalize(colpart, colpart + N, 2N, ceil(M/128), M, N, ...)).
 *   C2  optional second output [M][n2] row stride ldc2 (n2, ldc2 multiples of 8, n2 <= N): a compact copy of columns
 *       [0, n2) of C.  The next bottleneck's gate-shift reads only that channel slice (shift.py:46-93), three times; out of
 *       the channels-last map every such read drags whole rows' cache lines along (measured 4.5x the slice's bytes).
 *       c2_pre (tdeed_gemm_fwd only): C2 receives the value before residual and activation and columns [0, n2) of C keep the
 *       residual alone -- the input gradient of a gate-shifted conv1 (shift.py:89-93 backwards): those columns belong to the
 *       gate-shift module's backward, the block's shortcut gradient R joins the rest in this epilogue. */
int tdeed_gemm_fwd(const void* A, long lda, const void* A0, long lda0, int k0,
                   const float* a_scale, int a_scale_rows, int M, int K, int N, const void* W,
                   long ldw, const float* scale, const float* shift, const void* R, long ldr,
                   int act, void* C, long ldc, int gather_stride, int gather_hi, int gather_wi,
                   int gather_ho, int gather_wo, float* colpart, void* C2, long ldc2, int n2, int c2_pre, int dtype,
                   void* stream);

/* Weight-stationary variant of the same contraction for narrow layers (whole W in LDS, activations
 * streamed global->registers in MFMA fragment shape, persistent blocks; see gemm.hip).  Same
 * semantics and arguments as tdeed_gemm_fwd except that the weights arrive pre-packed:
 * Wfrag = tdeed_amd.packing.pack_ws_weights(W): [2*ceil(N/32)][ceil(K/(4*epc))][64 lanes][16 B], rows
 * permuted so that each lane owns 8 consecutive output channels.  tdeed_gemm_ws_fits() tells whether
 * (K, N, dtype) fits (LDS budget 64 KB). */
int tdeed_gemm_ws_fits(int K, int N, int dtype);
int tdeed_gemm_ws_fwd(const void* A, long lda, const void* A0, long lda0, int k0,
                      const float* a_scale, int a_scale_rows, int M, int K, int N, const void* Wfrag,
                      const float* scale, const float* shift, const void* R, long ldr, int act,
                      void* C, long ldc, int gather_stride, int gather_hi, int gather_wi,
                      int gather_ho, int gather_wo, void* C2, long ldc2, int n2, int dtype, void* stream);

/* conv3 of a bottleneck whose shortcut is a 1x1 conv (stride 1|2), the two launches
 *   sc = bf16((gather(As) @ Ws^T) * sscale + sshift);  C = act((A' @ W^T) * scale + shift + sc)
 * as one: the shortcut product goes into a second accumulator set, is scaled, shifted and rounded to bf16 in registers and
 * takes the residual's place -- bit-identical to tdeed_gemm_ws_fwd twice, and the shortcut map never exists.  Arguments of
 * tdeed_gemm_ws_fwd without R / ldr; As [rows of the block's input][ldas], Ks its channels, Wsfrag = pack_ws_weights(Ws)
 * (same N); the gather geometry applies to As only (A is not gathered).  bf16; both weights sit in LDS (up to 80 KB =
 * two workgroups per CU).  tdeed_gemm_ws_sc_fits: (ceil(K/32), ceil(Ks/32)) is (2, 1) or (5, 2) and the weights fit. */
int tdeed_gemm_ws_sc_fits(int K, int Ks, int N, int dtype);
int tdeed_gemm_ws_sc_fwd(const void* A, long lda, const void* A0, long lda0, int k0, const float* a_scale,
                         int a_scale_rows, int M, int K, int N, const void* Wfrag, const float* scale,
                         const float* shift, const void* As, long ldas, int Ks, const void* Wsfrag,
                         const float* sscale, const float* sshift, int act, void* C, long ldc, int gather_stride,
                         int gather_hi, int gather_wi, int gather_ho, int gather_wo, void* C2, long ldc2, int n2,
                         int dtype, void* stream);

/* ---- grouped 3x3 conv + BN + ReLU + SE squeeze ---------------------------------------------
 * timm Bottleneck.conv2 (groups = C/gw, stride 1|2, pad 1) + BN(eval) + ReLU, and the SE
 * squeeze (sum over H,W) of its output.  x: [N][Hi][Wi][C], y: [N][Ho][Wo][C], gw in {8,16}.
 *   w      fp32 [G][9][gw_in][gw_out] (tap-major repack of Conv2d.weight [C][gw][3][3]); used by the
 *          VALU kernel (TDEED_F32, or bf16 when wfrag is NULL).
 *   wfrag  bf16 MFMA operand fragments [ceil4(C/16)][5][64][8] (see tdeed_amd.packing.pack_gconv_frags);
 *          TDEED_BF16 only: implicit GEMM on v_mfma_f32_16x16x32_bf16 from an LDS-staged halo band.
 *   pooled fp32 [N][parts][C]: per-band partial SUMS of y over pixels, parts =
 *          tdeed_gconv3x3_parts(Hi, Wi, C, stride, dtype) (1 on the VALU path).
 *   pooled_sq  optional (bf16 MFMA path), same shape: partial sums of y^2 -- with pooled the BatchNorm batch statistics
 *          of the raw conv output (tdeed_bn_finalize(pooled, pooled_sq, C, N*parts, N*Ho*Wo, C, ...)). */
int tdeed_gconv3x3_parts(int Hi, int Wi, int C, int stride, int dtype);
int tdeed_gconv3x3_mfma_fits(int Hi, int Wi, int C, int stride);   /* 1: the bf16 MFMA kernel (wfrag, in_a) serves it */
/*   in_a, in_b  optional fp32 [C] (bf16 MFMA path, training): x is the RAW output of the conv in front and
 *          relu(in_a[c] * x + in_b[c]) -- the BatchNorm(batch statistics) + ReLU between the two convs -- is applied while
 *          the band is staged, so the post-BN map is never written; bit-identical to running on the materialised map. */
int tdeed_gconv3x3_fwd(const void* x, int N, int Hi, int Wi, int C, int gw, int stride,
                       const float* w, const void* wfrag, const float* scale, const float* shift,
                       void* y, float* pooled, float* pooled_sq, const float* in_a, const float* in_b,
                       int relu /* 0: y = conv*scale+shift (training: raw map for the batch statistics) */, int dtype,
                       void* stream);

/* Split-K form of the contraction for the short sequences of the SGP encoder-decoder (a few hundred rows, K up to
 * 6C; bf16): C = act((A . W^T) * scale + shift + R).  Two launches: S = tdeed_gemm_splitk_splits(K) partial products
 * into `workspace` (fp32, S*M*N elements, caller-owned), then a reduce + epilogue pass. */
int tdeed_gemm_splitk_splits(int K);
int tdeed_gemm_splitk_partials(const void* A, long lda, int M, int K, int N, const void* W, long ldw, float* workspace,
                               void* stream);   /* the partial products only: workspace [splits(K)][M][N] fp32 */
int tdeed_gemm_splitk_fwd(const void* A, long lda, int M, int K, int N, const void* W, long ldw, const float* scale,
                          const float* shift, const void* R, long ldr, int act, void* C, long ldc,
                          float* workspace, void* stream);

/* SE excitation on the MFMA pipe (bf16 weights as A-operand fragments [ceil(R/16)][ceil(C/32)][64][8] and
 * [ceil(C/16)][ceil(R/32)][64][8], tdeed_amd.packing.pack_se_mfma); 16 frames per workgroup; same contract as
 * tdeed_se_gate_bf16_fwd.  tdeed_se_gate_mfma_fits(C, R) != 0 tells whether the shape is covered (C <= 384, R <= 96). */
int tdeed_se_gate_mfma_fits(int C, int R);
int tdeed_se_gate_mfma_fwd(const float* pooled, int n_parts, float inv_cnt, int N, int C, int R, const void* w1f,
                           const float* b1, const void* w2f, const float* b2, float* gate, void* stream);

/* Register-stationary form of the same contraction for K = N = 320 over many rows (conv1 / conv3 of the s3 blocks of
 * RegNetY-800MF): the whole weight matrix lives in the registers of a 10-wave workgroup, the activations cross the chip once
 * (64-row tiles through LDS).  Arguments as tdeed_gemm_ws_fwd (Wfrag from pack_ws_weights, bf16) without the row gather;
 * a_scale_rows >= 64.  tdeed_gemm_rs_fits(M, K, N) != 0 tells whether the shape is covered. */
int tdeed_gemm_rs_fits(int M, int K, int N);
int tdeed_gemm_rs_fwd(const void* A, long lda, const void* A0, long lda0, int k0, const float* a_scale, int a_scale_rows,
                      int M, int K, int N, const void* Wfrag, const float* scale, const float* shift, const void* R, long ldr,
                      int act, void* C, long ldc, void* C2, long ldc2, int n2, void* stream);

/* the same contraction as the training forward runs it: raw output + the BatchNorm statistics of that output, one partial
 * row per persistent workgroup: colpart fp32 [tdeed_gemm_rs_grid(M)][2][N] (column sums | sums of squares) */
int tdeed_gemm_rs_grid(int M);
int tdeed_gemm_rs_stats_fwd(const void* A, long lda, const void* A0, long lda0, int k0, int M, int K, int N, const void* Wfrag,
                            void* C, long ldc, float* colpart, void* stream);

/* conv1 (1x1 + BN + ReLU, with the gate-shift splice of shift.py:89-93) IN FRONT of the grouped 3x3 of the same timm
 * Bottleneck, one launch: the y1 band the grouped conv reads is computed in LDS from the block input, the y1 map (the
 * largest intermediate of a stride-2 block) never exists.  bf16.  x [N][Hi][Wi][Cin]; G optional [N*Hi*Wi][Fp]; w1f: conv1
 * weight [C][Cin] as MFMA A-operand fragments [tdeed_c1_gconv_slab_tiles()][ceil(Cin/32)][64][8] (zero padded to whole
 * slabs); s1 / h1: its folded BatchNorm; wfrag / scale / shift / y / pooled as tdeed_gconv3x3_fwd (ReLU applied).
 * Bit-identical to tdeed_gemm_fwd (or tdeed_gemm_ws_fwd) followed by tdeed_gconv3x3_fwd.  tdeed_c1_gconv_fits: Cin <= 64, or 97..160 (k-steps of 32: 1, 2, 4, 5). */
/* diagnostic: int64 [workgroups][8] phase time stamps of tdeed_c1_gconv_fwd (wall_clock64, 10 ns ticks; 0 start, 1 weights
 * requested + halo zeroed, 2 wave 0's conv1 tiles done, 3 barrier, 4 grouped conv set up, 5 its tiles multiplied and stored,
 * 6 squeeze sums stored); null switches it off */
int tdeed_c1_gconv_set_debug(void* buf);
int tdeed_c1_gconv_fits(int Hi, int Wi, int Cin, int C, int stride);
int tdeed_c1_gconv_slab_tiles(int Hi, int Wi, int C, int stride);
int tdeed_c1_gconv_fwd(const void* x, const void* G, int Fp, int N, int Hi, int Wi, int Cin, int C, int gw, int stride,
                       const void* w1f, const float* s1, const float* h1, const void* wfrag, const float* scale,
                       const float* shift, void* y, float* pooled, void* stream);
/* tdeed_c1_gconv_fwd has two forms with the same bits: one workgroup per (frame, band, channel slab), and the slab loop --
 * one workgroup per (frame, band) that keeps its x / G fragments in registers and walks the slabs.
 * tdeed_c1_gconv_slab_loop_fits: the slab loop exists for the shape (stride 2, several slabs, Cin in 33..64 or 129..160, a
 * wave's share of the band's pixel tiles fits its registers); which fitting shapes take it is routed per instance from
 * measurements.  tdeed_c1_gconv_set_form (tests, tools): -1 as routed (default), 0 per slab everywhere, 1 the slab loop
 * wherever it fits.  tdeed_c1_gconv_workgroups: the grid of tdeed_c1_gconv_fwd for N frames under the form in force (0: not
 * served).  In the slab loop the time stamps are: 1 prologue (halo, fold, everything requested), 2 slab 0's conv1, 3 barrier,
 * 4 slab 0's grouped conv, 5 the other slabs, 6 = 5. */
int tdeed_c1_gconv_set_form(int form);
int tdeed_c1_gconv_slab_loop_fits(int Hi, int Wi, int Cin, int C, int stride);
int tdeed_c1_gconv_workgroups(int N, int Hi, int Wi, int Cin, int C, int stride);

/* tdeed_c1_gconv_fwd of a stride-2 block whose input is not in memory: the launch also computes the producer's conv3 (Cp <=
 * 32 channels in and out: one k-step) per pixel tile in front of conv1, from its operand y2p, its shortcut map scp (both
 * [N][Hi][Wi][Cp] bf16), its SE gate [N][Cp] fp32, its weights w3f = pack_ws_weights(W3) and its fold s3 / h3 (ReLU applied).
 * xs2 optional [N][ceil(Hi/2)][ceil(Wi/2)][Cp]: the producer's output at even rows and columns (what the block's shortcut
 * conv reads).  The rest as tdeed_c1_gconv_fwd with Cin = Cp, stride 2.  Bit-identical to tdeed_gemm_ws_fwd (a_scale = gate,
 * R = scp, ReLU) followed by tdeed_c1_gconv_fwd; the producer's output map never exists.
 * tdeed_c1_gconv_c3in_fits: Cp in 8..32, C <= 64 (one channel slab), tdeed_c1_gconv_fits(Hi, Wi, Cp, C, 2), and a frame of the
 * operands below 2^31 bytes (Hi * Wi * Cp * 2: the kernel addresses a frame with 32-bit byte offsets). */
int tdeed_c1_gconv_c3in_fits(int Hi, int Wi, int Cp, int C);
int tdeed_c1_gconv_c3in_fwd(const void* y2p, const void* scp, const float* gate, const void* w3f, const float* s3,
                            const float* h3, void* xs2, int N, int Hi, int Wi, int Cp, int C, int gw, const void* w1f,
                            const float* s1, const float* h1, const void* wfrag, const float* scale, const float* shift,
                            void* y, float* pooled, void* stream);
/* tdeed_c1_gconv_c3in_fwd is one kernel, the band walk: one workgroup per (frame, run of `walk` consecutive bands) that runs
 * the prologue once per run, copies the input row two adjacent bands share inside LDS instead of computing it twice, and
 * requests the next band's operands under the grouped conv.  The bits are the same at every run length.
 * tdeed_c1_gconv_c3in_walk: the routed run length for the shape (at most the frame's band count; a function of the shape
 * alone, never of N; 0: not served).  tdeed_c1_gconv_c3in_set_walk (tests, tools): 0 as routed (default), k >= 1 runs of k
 * bands (clamped to the frame's band count; 1: runs of one band, a workgroup per (frame, band)); a negative value is an
 * error.  tdeed_c1_gconv_c3in_workgroups: the grid of tdeed_c1_gconv_c3in_fwd for N frames under the run length in force (0:
 * not served). */
int tdeed_c1_gconv_c3in_set_walk(int walk);
int tdeed_c1_gconv_c3in_walk(int Hi, int Wi, int Cp, int C);
int tdeed_c1_gconv_c3in_workgroups(int N, int Hi, int Wi, int Cp, int C);

/* A whole stride-1 RegNetY bottleneck with identity shortcut on a small map in ONE launch (timm Bottleneck.forward:
 * conv1 -> conv2 -> se -> conv3 + shortcut -> ReLU, with the gate-shift splice of shift.py:89-93 on conv1's operand;
 * SURVEY §8 a2 / a3): the frames of a workgroup stay in LDS, only x and the output cross HBM.  bf16.
 *   x [N][h][w][C]; G optional [N*h*w][Fp] compact gate-shift output replacing channels [0, Fp) of conv1's operand (the
 *   residual is x itself); w1f / w3f: conv weights [C][C] as MFMA A-operand fragments [ceil(C/16)][ceil(C/32)][64][8]
 *   (tdeed_amd.packing.pack_mfma_frags); w2f as for tdeed_gconv3x3_fwd (pack_gconv_frags, group width 8 or 16); se_w1f /
 *   se_w2f / R as for tdeed_se_gate_mfma_fwd; s*, h*: folded BatchNorm scale / shift; out [N][h][w][C]; out2 optional
 *   [N*h*w][n2] compact copy of channels [0, n2) (the next block's gate-shift slice).
 * Bit-identical to tdeed_gemm_fwd -> tdeed_gconv3x3_fwd -> tdeed_se_gate_mfma_fwd -> tdeed_gemm_fwd on the same operands.
 * tdeed_bneck_fits: 7x7x368 (two frames per workgroup) and 14x14x152 are the shapes it was built for.
 * tdeed_bneck_set_debug(buf): diagnostic, int64 [workgroups][16] phase time stamps (null switches it off). */
int tdeed_bneck_fits(int h, int w, int C, int R);
int tdeed_bneck_set_debug(void* buf);
int tdeed_bneck_fwd(const void* x, const void* G, int Fp, int N, int h, int w, int C, const void* w1f, const float* s1,
                    const float* h1, const void* w2f, const float* s2, const float* h2, const void* se_w1f,
                    const float* se_b1, const void* se_w2f, const float* se_b2, int R, const void* w3f, const float* s3,
                    const float* h3, void* out, void* out2, int n2,
                    int w2_tap_major /* k-slot order of w2f: 1 = packing.pack_gconv_frags(tap_major=True), the conflict-free
                                        order of this launch (group width 8); 0 = the order tdeed_gconv3x3_fwd reads */,
                    void* stream);
/* The same block behind a gate-shift-fuse site (impl/gsf.py:74-93) with the site's last launch -- fusion weights + blend,
 * tdeed_gsf_blend_src_fwd -- done inside the frame load: gx [N][h*w][ldx] is the slice's source (the block input, or the
 * compact copy of its first Fp channels), gate / ysum / xsum are tdeed_gsf_gate_fwd's outputs for the N = B * T frames, cw* / cb*
 * the two fusion convs.  out == tdeed_bneck_fwd(x, G = tdeed_gsf_blend_src_fwd(gx, ...)), bit for bit.
 * Q (optional, tdeed_bneck_qtail_fits): the tap maps [N][h*w][6] of the NEXT block's gate-shift site (impl/gsf.py:49-52, the
 * conv3d as three 2-D convs per frame), made from this block's output rows while they are in LDS -- what the first launch of
 * tdeed_gsf_gate_fwd computes from `out`, as a 1x1 contraction to per-tap sums plus nine fp32 adds (same products, another
 * summation order: equal to fp32 rounding); the site then runs tdeed_gsf_gate_sums_fwd only.  q_wqf: the site's weights as
 * packing.pack_gsf_p_frags lays them out; q_bn [2][8 * ceil(q_F / 8)]: its folded BatchNorm3d scale | shift, zeros behind
 * channel q_F. */
int tdeed_bneck_qtail_fits(int h, int w, int C, int F);
int tdeed_bneck_gs_fwd(const void* x, const void* gx, int ldx, const float* gate, const float* ysum, const float* xsum,
                       const float* cw1, const float* cb1, const float* cw2, const float* cb2, int T, int F, int Fp, int N,
                       int h, int w, int C, const void* w1f, const float* s1, const float* h1, const void* w2f,
                       const float* s2, const float* h2, const void* se_w1f, const float* se_b1, const void* se_w2f,
                       const float* se_b2, int R, const void* w3f, const float* s3, const float* h3, void* out, void* out2,
                       int n2, int w2_tap_major, const void* q_wqf, const float* q_bn, int q_F, float* Q, void* stream);


/* ---- SE excitation: gate = sigmoid(W2 relu(W1 mean + b1) + b2) -----------------------------
 * timm SEModule fc1/ReLU/fc2/sigmoid.  pooled: fp32 [N][n_parts][C] partial sums, mean = inv_cnt *
 * sum over parts; gate: fp32 [N][C]; w1t [C][R] (fc1.weight transposed), w2t [R][C] (fc2.weight transposed). */
int tdeed_se_gate_fwd(const float* pooled, int n_parts, float inv_cnt, int N, int C, int R,
                      const float* w1t, const float* b1, const float* w2t, const float* b2,
                      float* gate, void* stream);

/* Same excitation with bf16 weights (throughput mode): w1p bf16 [C][ceil8(R)] (fc1.weight^T zero padded),
 * w2p bf16 [R][C] (fc2.weight^T) = tdeed_amd.packing.pack_se_bf16. */
int tdeed_se_gate_bf16_fwd(const float* pooled, int n_parts, float inv_cnt, int N, int C, int R,
                           const void* w1p, const float* b1, const void* w2p, const float* b2,
                           float* gate, void* stream);

/* ---- Gate-Shift(-Fuse) (model/impl/gsf.py:38-93, model/impl/gsm.py:89-116, eval BN) ------------
 * x: [B*T][h][w][C] (first F channels are gated).  Three launches:
 *  gate:   BN3d+ReLU+Conv3d(3x3x3, groups 2)+tanh -> gate fp32 [B*T][h][w][2]; also
 *          ysum[B*T][F] = sum_hw gate*x, xsum[B*T][F] = sum_hw x (fp32).  Two kernels inside: per-frame
 *          partial sums Q (each frame read once), then the temporal combine + tanh + spatial sums.
 *  weight: GSF only: fusion weight fw[B][F][T] = sigmoid(Conv2d(2->1,3x3) over the (c,t) plane
 *          of [mean shifted y ; mean r]) (gsf.py:61-78).
 *  apply:  out[B*T][h][w][Fp] : channels [0,F) = interleave(shift(y)*fw + r*(1-fw)) (GSM: fw==1
 *          i.e. shift(y)+r), channels [F,Fp) copied from x (Fp = F rounded up to 8). */
int tdeed_gsf_gate_fwd(const void* x, int B, int T, int h, int w, int C, int F,
                       const float* bn_scale, const float* bn_shift,
                       const float* wq /*[27][F] tap-major conv3D weight (VALU path)*/,
                       const void* wqf /*bf16 MFMA fragments, packing.pack_gsf_q_frags; NULL => VALU*/,
                       const float* b3d /*[2]*/,
                       float* Q /*scratch fp32 [B*T][h][w][6]*/, float* gate, float* ysum, float* xsum,
                       int dtype, void* stream);
/* The second launch of tdeed_gsf_gate_fwd alone (gates + spatial sums), for a site whose tap maps Q were made by the launch in
 * front of it (tdeed_bneck_gs_fwd's Q).  bf16. */
int tdeed_gsf_gate_sums_fwd(const void* x, int B, int T, int h, int w, int C, int F, const float* b3d, const float* Q,
                            float* gate, float* ysum, float* xsum, void* stream);
int tdeed_gsf_weight_fwd(const float* ysum, const float* xsum, int B, int T, int F, int hw,
                         const float* cw1 /*[2][3][3]*/, const float* cb1, const float* cw2,
                         const float* cb2, float* fw /*[B][F][T]*/, void* stream);
int tdeed_gsf_apply_fwd(const void* x, const float* gate, const float* fw /*NULL => GSM*/, int B,
                        int T, int h, int w, int C, int F, int Fp, void* out, int dtype,
                        void* stream);

/* weight + apply in one launch (GSF): every frame's block evaluates its own fusion weights from ysum/xsum first. */
int tdeed_gsf_apply_fused_fwd(const void* x, const float* gate, const float* ysum, const float* xsum,
                              const float* cw1, const float* cb1, const float* cw2, const float* cb2, int B,
                              int T, int h, int w, int C, int F, int Fp, void* out, int dtype, void* stream);
/* the same launch with the output left in SOURCE channel order (impl/gsf.py:79-91 without the final `c = i*(F/4)+j -> 2j+i`
 * interleave; bf16 only): for a caller that folds the interleave into the columns of the 1x1 conv reading the slice
 * (engine.gs_source_order_columns); everything stays in registers, one memory round trip per frame. */
int tdeed_gsf_blend_src_fwd(const void* x, const float* gate, const float* ysum, const float* xsum,
                            const float* cw1, const float* cb1, const float* cw2, const float* cb2, int B,
                            int T, int h, int w, int C, int F, int Fp, void* out, int dtype, void* stream);

/* ---- global average pool + positional encoding (model.py:133-137) --------------------------
 * x: [B*T][hw][C] -> feat [B][T][C] = mean_hw(x) + temp_enc[t][c] (temp_enc fp32 [T][C]).  rowstat (optional, fp32
 * [B*T][2]): LayerNorm mean / rstd over C of every stored feature row, for tdeed_sgp_front_fwd of the first SGP block. */
int tdeed_avgpool_posenc_fwd(const void* x, int B, int T, int hw, int C, const float* temp_enc,
                             void* feat, float* rowstat, int dtype, int dtype_out /* feat: dtype, or TDEED_F32 */, void* stream);

/* ---- SGP pyramid pieces (model/modules.py:58-363), NTC layout ------------------------------- */
/* channel LayerNorm of every row (modules.py:320-363): y[r][c] = (x-mu)/sqrt(var+eps)*w[c]+b[c];
 * rows = B*T, row strides ldx / ldy (elements) so the result can land in a slab of the mixer's
 * concat buffer. */
int tdeed_layernorm_fwd(const void* x, long ldx, int rows, int C, const float* w, const float* b,
                        float eps, void* y, long ldy, int dtype, void* stream);
/* SGPBlock front half (modules.py:161-184): given o = LN(x):
 *   y = x + fc(o)*relu(gfc(mean_T o)) + (convw(o)+convkw(o))*psi(o) + o
 * dw: fp32 packed per channel [C][2*ks+up+2]: psi[ks], convw[ks], convkw[up], fc, global_fc;
 * db: fp32 [5][C] biases in the order psi, convw, convkw, fc, global_fc. */
int tdeed_sgp_branch_fwd(const void* o, const void* x, int B, int T, int C, int ks, int up,
                         const float* dw, const float* db, void* y, int dtype, void* stream);
/* SGPMixer front half (modules.py:286-308): zn = LN1(z) already sits in slab 4 of cat, xn = LN2(x)
 * at T_lo.  Upsamples xn (linear, align_corners) and fills slabs 0-3 and 5 of
 * cat [B][T_hi][6C] = (out1,out2,out3,out4,zn,xu).  dw1/db1, dw2/db2 as in sgp_branch. */
int tdeed_mixer_branch_fwd(const void* xn, int B, int T_hi, int T_lo, int C, int ks, int up,
                           const float* dw1, const float* db1, const float* dw2,
                           const float* db2, void* cat, int dtype, void* stream);
/* ---- fused SGP launches (sgp_fused.hip): a block = sgp_front + two contractions, a mixer = mixer_front + three.
 * sgp_front:   y = x + LN(x) + fc*phi + (convw+convkw)*psi   (modules.py:159-184; LayerNorm 320-363 computed in-kernel)
 * mixer_front: cat [B][T_hi][6C] = (out1,out2,out3,out4,LN1(z),up(LN2(x_lo)))   (modules.py:286-308)
 * (out = y + mlp(GroupNorm16(y)) and concat_fc: tdeed_sgp_gemm_* below, csrc/sgp_gemm.hip) */
/* chsum (optional, fp32 [B][C][2]): per clip and channel the sum and sum of squares over T of the stored y, which
 * tdeed_sgp_gemm_gn_gelu takes for its GroupNorm statistics */
/* rowstat* (optional, fp32 [rows][2] = LayerNorm mean, rstd of every input row, as tdeed_avgpool_posenc_fwd leaves them):
 * taken instead of re-deriving the statistics from the clip's (T x C) slab */
/* rowstat*_parts: 0 = the (mean, rstd) form above; n > 0 = [n][rows][2] partial (sum, sum of squares) of each row over the n
 * column tiles of the tdeed_sgp_gemm_residual launch that stored the rows (summed in order; mean / rstd derived here).
 * dtype_cat (mixer): the six slabs may be stored as bf16 while z / x_lo are fp32 (fp32 residual stream, bf16 contraction). */
/* diagnostic: int64 [workgroups][16] phase time stamps of tdeed_sgp_front_fwd (wall_clock64, 10 ns ticks; slots 0..5 = start,
 * loads issued + row statistics, tile in LDS, LayerNorm applied, branches done, stored); null switches it off */
int tdeed_sgp_front_set_debug(void* buf);
int tdeed_sgp_front_fwd(const void* x, int B, int T, int C, int ks, int up, const float* ln_w, const float* ln_b, float eps,
                        const float* dw, const float* db, void* y, float* chsum, const float* rowstat, int rowstat_parts,
                        void* y16 /* optional, dtype fp32 only: a bf16 copy of y (the fc1 operand of wide models) */,
                        int dtype, void* stream);
int tdeed_mixer_front_fwd(const void* z, const void* xlo, int B, int T_hi, int T_lo, int C, int ks, int up,
                          const float* ln1_w, const float* ln1_b, const float* ln2_w, const float* ln2_b, float eps,
                          const float* dw1, const float* db1, const float* dw2, const float* db2, void* cat,
                          const float* rowstat_z, int rowstat_z_parts, const float* rowstat_x, int rowstat_x_parts,
                          int dtype, int dtype_cat, void* stream);
/* nn.GroupNorm(G, C) over (C/G x T) per clip (modules.py:115,186): x,y [B][T][C]. */
int tdeed_groupnorm_fwd(const void* x, int B, int T, int C, int G, const float* w, const float* b,
                        float eps, void* y, int dtype, void* stream);
/* nn.AdaptiveMaxPool1d over T (modules.py:64,76): [B][T_in][C] -> [B][T_out][C]. */
int tdeed_maxpool_fwd(const void* x, int B, int T_in, int T_out, int C, void* y, int dtype,
                      void* stream);
/* the same pooling with the LayerNorm statistics (mean, rstd over C, eps inside the sqrt; modules.py:353-357) of every pooled
 * row in rowstat [B*T_out][2] -- what tdeed_sgp_front_fwd of the next block takes instead of re-deriving them */
int tdeed_maxpool_rowstat_fwd(const void* x, int B, int T_in, int T_out, int C, void* y, float* rowstat, float eps, int dtype,
                              void* stream);

/* ---- heads (modules.py:366-387, model.py:141-146), eval (no dropout) ------------------------
 * x [rows][C]; w fp32 [n_out][C], b [n_out]; out fp32 [rows][n_out] (class logits and the
 * displacement column are rows of the same matrix: one read of x). */
int tdeed_heads_fwd(const void* x, int rows, int C, const float* w, const float* b, int n_out,
                    float* out, int dtype, void* stream);

/* ---- loss (model.py:208-211, 308-319) -------------------------------------------------------
 * Weighted CE (hard int64 labels, or soft [rows][K1] when soft!=NULL) + MSE(displ, labelD).
 * out fp32 [3]: total, ce, mse.  logits fp32 [rows][ld] (first K1 columns), displ = column
 * `displ_col` of the same matrix (or <0 for none). */
int tdeed_loss_fwd(const float* logits, int rows, int ld, int K1, const int64_t* hard,
                   const float* soft, const float* cls_w, int displ_col, const float* labelD,
                   float* out, void* stream);

/* ---- training path, first pieces (a13 backward, a14): see train.hip ------------------------------------------
 * loss_bwd: dhead = grad_scale * d(CE + MSE)/d(head_out), same arguments as tdeed_loss_fwd; columns that do not
 *           take part in the loss get 0.
 * heads_bwd: FCLayers backward (modules.py:366-376): dx (activation dtype, may be NULL), dw fp32 [n_out][C],
 *           db fp32 [n_out]; workspace of tdeed_heads_bwd_workspace() bytes (deterministic two-stage reduction).
 * adamw_step: torch.optim.AdamW update (modules.py:37-39, defaults betas (0.9,0.999) eps 1e-8 wd 0.01) fused over
 *           one flat fp32 buffer; `step` counts from 1; grad_scale pre-multiplies the gradient (1/world, 1/acc...). */
int tdeed_loss_bwd(const float* head_out, int rows, int ld, int K1, const int64_t* hard, const float* soft,
                   const float* cls_w, int displ_col, const float* labelD, float grad_scale, float* dhead,
                   void* stream);
/* joint-dataset double head (model.py:278-306): per-clip CE on the clip's own class slice (K1a | K1b columns, dataset[i] in
 * {1,2}, labels of dataset 2 shifted by K1a), mean over clips, + displacement MSE.  out [3] and/or dhead (either NULL).
 * hard: int64 [B*T], or soft: fp32 [B*T][K1a+K1b] label distributions (mixup with the double head: the 3-D label branch
 * of model.py:286-300).  Labels outside [0, K) of their slice are never used as an index: the loss comes back NaN
 * (the same holds for tdeed_loss_fwd / tdeed_loss_bwd; torch's cross_entropy raises in that case). */
int tdeed_loss2(const float* head_out, int B, int T, int ld, int K1a, int K1b, const int64_t* dataset, const int64_t* hard,
                const float* soft, const float* cls_w, int displ_col, const float* labelD, float grad_scale, float* out,
                float* dhead, void* stream);
/* distillation (opt-in): total = (1-alpha) CE + MSE + alpha KD + displ_weight KDdispl, value and gradient in one launch.
 * CE / MSE are the terms of tdeed_loss_fwd / tdeed_loss_bwd (alpha = displ_weight = 0 gives their bits);
 * KD = temperature^2 / rows * sum_r KL(softmax(t_r / temperature) || softmax(s_r / temperature)) with s = head_out[r][0..K1)
 * and t = teacher[r][0..K1), read in place from the teacher's own head buffer (row stride ld_t, displacement column
 * displ_col_t or <0); KDdispl = mean_r (d_s - d_t)^2 when both displacement columns exist, else 0 (displ_weight > 0 is
 * then an argument error).  out5: total, ce, mse, kd, kd_displ.  dhead [rows][ld] may be NULL (value only).  Nothing is
 * clamped: a non-finite teacher logit gives a non-finite kd and gradient row. */
int tdeed_loss_kd(const float* head_out, int rows, int ld, int K1, const int64_t* hard, const float* soft,
                  const float* cls_w, int displ_col, const float* labelD, const float* teacher, int ld_t, int displ_col_t,
                  float alpha, float temperature, float displ_weight, float grad_scale, float* out5, float* dhead,
                  void* stream);
/* loss options (opt-in): label smoothing, a focal exponent and free per-class weights cls_w[K1] on the classification term,
 * value and gradient in one launch; with teacher != NULL the distillation terms of tdeed_loss_kd on top, with teacher ==
 * NULL kd = kd_displ = 0 and alpha / displ_weight must be 0 (ld_t, displ_col_t, temperature are then ignored).
 * ce = sum_r sum_c w_c t'_c (1 - p_c)^focal_gamma (-log p_c) / den,  t' = (1 - label_smoothing) t + label_smoothing / K1
 * (t: one-hot of the hard label or the soft row), den = sum_r w[y_r] (hard) or rows (soft); focal_gamma = 0 is
 * F.cross_entropy(weight=, label_smoothing=).  label_smoothing = focal_gamma = 0 gives the bits of tdeed_loss_kd, without
 * a teacher those of tdeed_loss_fwd + tdeed_loss_bwd.  out5: total, ce, mse, kd, kd_displ.  dhead may be NULL.
 * Argument errors: label_smoothing outside [0, 1], focal_gamma negative or not finite, and those of tdeed_loss_kd. */
int tdeed_loss_opt(const float* head_out, int rows, int ld, int K1, const int64_t* hard, const float* soft,
                   const float* cls_w, int displ_col, const float* labelD, const float* teacher, int ld_t, int displ_col_t,
                   float alpha, float temperature, float displ_weight, float label_smoothing, float focal_gamma,
                   float grad_scale, float* out5, float* dhead, void* stream);
long tdeed_heads_bwd_workspace(int rows, int C, int n_out);
int tdeed_heads_bwd(const float* dout, const void* x, int rows, int C, const float* w, int n_out, void* dx,
                    float* dw, float* db, void* workspace, int dtype, void* stream);
int tdeed_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, float lr,
                     float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                     void* stream);

/* ---- guarded optimizer step (opt-in; see train.hip) -------------------------------------------------------------
 * What the reference's GradScaler did for the optimizer (modules.py:390-404: scaler.step() leaves the optimizer and
 * its step count untouched when a gradient holds an inf or a NaN) and clip_grad_norm_'s rule, with no host
 * synchronisation and legal under stream capture.
 *
 * grad_guard: statistics of the flat fp32 gradient buffer, two launches.  Pass one sums g*g in binary64 (the square of an
 *   fp32 value is exact there, and up to 2^31 of them cannot overflow, so the sum is finite exactly when every element
 *   is: a buffer of FLT_MAX counts as finite) into one partial per workgroup in `ws`; pass two (one workgroup) folds the
 *   partials in a fixed order and writes the record.  No atomics: the bits do not depend on which workgroup runs when.
 *   `ws`: tdeed_grad_guard_ws_bytes(n) bytes (at most 4096 * 8), 8-byte aligned.  `guard`: the caller's record, 32 bytes,
 *   16-byte aligned, zero before the first call:
 *       offset  0  double  sumsq      this call's sum of squares of the raw buffer (before any grad_scale)
 *       offset  8  int32   nonfinite  this call: 1 when the buffer holds an inf or a NaN, else 0
 *       offset 12  int32   skipped    cumulative: pass two adds `nonfinite` to it when skip_nonfinite is set; nothing else
 *                                     writes it
 *       offset 16  16 bytes reserved, written as zero
 * adamw_step_guarded: tdeed_adamw_step behind that record (the same update code).
 *   skip_nonfinite != 0 and nonfinite != 0: the launch writes nothing (param, exp_avg, exp_avg_sq keep their bits).
 *   max_grad_norm > 0: grad_scale is multiplied by min(1, max_grad_norm / (grad_scale * sqrt(sumsq) + 1e-6)), torch's
 *     clip_grad_norm_ applied to the norm of the gradient AdamW sees (the mean over ranks and micro-batches); a coefficient
 *     of 1 leaves grad_scale's bits alone; <= 0 means off.  With clipping on and skipping off a non-finite norm poisons
 *     the update exactly as clip_grad_norm_(error_if_nonfinite=False) followed by step() does.
 *   `step` stays the caller's count of ATTEMPTS (from 1).  While skipped == 0 the bias corrections are the host's, computed
 *     as tdeed_adamw_step computes them: on finite gradients without clipping the launch is bit-identical to
 *     tdeed_adamw_step.  Once skipped != 0 the effective step is step - skipped and the corrections come from the
 *     device's powf, which may differ from glibc's by a few ulp.
 *   The betas are fp32 here as in tdeed_adamw_step: beta2 = 0.999 arrives as float32(0.999) and 1 - beta2 is 9.99987e-04,
 *     so exp_avg_sq sits a relative 1.29e-05 from an optimizer run at the decimal 0.999 (param does not show it). */
long tdeed_grad_guard_ws_bytes(long n);
int tdeed_grad_guard(const float* grad, long n, int skip_nonfinite, void* guard, void* ws, void* stream);
int tdeed_adamw_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, float lr,
                             float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                             const void* guard, int skip_nonfinite, float max_grad_norm, void* stream);

/* ---- AdamW over runs: parameter groups and frozen tensors (opt-in; see train.hip) ---------------------------------
 * adamw_step_groups: the arguments of tdeed_adamw_step_guarded plus a device table of `nruns` (1 .. 16384) records that
 *   cut [0, n) into runs, 16 bytes each, 16-byte aligned, written by the caller in plain host code and uploaded once:
 *       offset  0  int32  end4      end of the run in 16-byte chunks (exclusive), ascending; the last run's is
 *                                   ceil(n / 4), so the scalar tail (n & 3) belongs to the last run
 *       offset  4  float  lr_scale  the run steps at lr * lr_scale (one fp32 product)
 *       offset  8  float  wd        the run's weight decay; < 0: the launch's weight_decay
 *       offset 12  int32  frozen    != 0: the run's param, grad, exp_avg, exp_avg_sq are neither loaded nor stored
 *   Every run boundary is a multiple of 4 elements, so no 16-byte chunk is split.  guard == NULL selects the unguarded
 *   form (skip_nonfinite / max_grad_norm are ignored); otherwise the record decides as in tdeed_adamw_step_guarded: a
 *   skipped step writes nothing in any run, and the clipping coefficient is the one global coefficient.  With
 *   lr_scale = 1, wd < 0 (or equal to weight_decay) and frozen = 0 in every run the launch is bit-identical to
 *   tdeed_adamw_step / tdeed_adamw_step_guarded.  The table's content cannot move a memory access: n bounds the buffers
 *   and nruns the table whatever the records hold. */
int tdeed_adamw_step_groups(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, float lr,
                            float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                            const void* guard, int skip_nonfinite, float max_grad_norm, const void* runs, int nruns,
                            void* stream);

/* ---- weight EMA inside the AdamW launch (opt-in; see train.hip) ----------------------------------------------------
 * adamw_step_ema: the arguments of tdeed_adamw_step_groups plus the shadow `ema` (n floats, 16-byte aligned), updated
 *   from the parameter the launch has just computed, while it is still in registers.  guard == NULL: the plain update;
 *   runs == NULL: no groups (nruns is ignored).  Per APPLIED step, all fp32, no contraction, three roundings:
 *       n_upd = (step - skipped) - ema_step0       (>= 1; skipped is the record's, 0 without a guard)
 *       d_n   = ema_warmup ? min(ema_decay, (1 + n_upd) / (10 + n_upd)) : ema_decay     (correctly rounded quotient)
 *       w     = 1 - d_n;   diff = p_new - e;   prod = w * diff;   e = e + prod
 *   A skipped step leaves the shadow untouched; a frozen run neither loads nor stores its shadow slice.  param, exp_avg and
 *   exp_avg_sq get the bits tdeed_adamw_step / _guarded / _groups would write.  0 < ema_decay < 1, ema_step0 >= 0,
 *   step - ema_step0 >= 1.
 * ema_tensors: the same update for tensors outside the flat buffer (BatchNorm running statistics).  `rows`: a device table
 *   of `nrows` (1 .. 65535) 16-byte rows, 16-byte aligned, written by the caller in plain host code and uploaded once:
 *       offset  0  const float*  src     the live tensor (4-byte aligned)
 *       offset  8  int32         offset  first element of the row in `shadow`
 *       offset 12  int32         count   elements
 *   `host_rows`: the caller's host copy of the same table; every row is checked against shadow_n before the launch (and
 *   bounded by it again on the device).  shadow[offset + i] is updated from src[i]; one workgroup per row; guard (may be
 *   NULL), skip_nonfinite, step and ema_step0 as above, so a skipped step leaves the shadow untouched. */
int tdeed_adamw_step_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, float lr,
                         float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                         const void* guard, int skip_nonfinite, float max_grad_norm, const void* runs, int nruns,
                         float* ema, float ema_decay, int ema_warmup, int ema_step0, void* stream);
int tdeed_ema_tensors(const void* rows, const void* host_rows, int nrows, float* shadow, long shadow_n, int step,
                      const void* guard, int skip_nonfinite, float ema_decay, int ema_warmup, int ema_step0, void* stream);

/* ---- post-proc (modules.py:406-426): softmax over the first K1 columns then scatter-max of
 * frame t onto clamp(t - rne(displ), 0, T-1).  scores fp32 [B][T][K1] (zero-initialised inside),
 * cls int64 [B][T] = argmax. */
int tdeed_process_prediction(const float* head_out, int B, int T, int ld, int K1, int displ_col,
                             float* scores, int64_t* cls, void* stream);

/* ---- utility ------------------------------------------------------------------------------- */
int tdeed_cast_f32_to_bf16(const float* src, void* dst, long n, void* stream);
/* the large dense weights' kernel copies in one launch: tab = device array of n entries of six 8-byte fields {const float* src
 * (an fp32 [R][C] matrix), long R, long C, void* dst ([R][C] in `dtype`, or NULL), void* dstT ([C][R] in `dtype`, or NULL),
 * long first_tile}; tiles = sum over the entries of ceil(R/32) * ceil(C/32), first_tile its running prefix */
int tdeed_multi_cast_transpose(const void* tab, int n, long tiles, int dtype, void* stream);
/* out[i] = idx[i] ? src[idx[i] - 1] : 0 for i < n (n a multiple of 8), out fp32 or bf16: all kernel-layout copies of the
 * master parameters (casts, transposes, MFMA fragment orders, zero pads) refreshed in one launch from a recorded index
 * table; replaces the per-tensor `.to(bf16)` / `.t().contiguous()` of a framework step. */
int tdeed_gather_cast(const float* src, const int* idx, long n, void* out, int dtype, void* stream);
int tdeed_fill_u8_hash(uint8_t* dst, long n, uint64_t seed, void* stream); /* synthetic clips */

/* ---- whole-video scoring (video.hip) ---------------------------------------------------------
 * video: uint8 [L][frame_bytes] resident on the device; starts: DEVICE int32[B] (first video frame of each clip, may be
 * negative or hang over the end).  clips_out[b][t] = video[starts[b] + t] when 0 <= starts[b] + t < L, else a zero frame
 * (dataset/frame.py:580-626 with pad=True).  16-byte accesses when frame_bytes % 16 == 0 and both buffers are 16-byte
 * aligned, a byte path otherwise.  B * T <= 65535. */
int tdeed_clip_gather_u8(const uint8_t* video, int L, long frame_bytes, const int* starts, int B, int T,
                         uint8_t* clips_out, void* stream);

/* ---- videos scored as one packed job: gathers, score stitching (video.hip), event spotting (spot.hip) --------------------
 * One video is a group of nv = 1 (seg_off = {0, L}, clip_off = {0, n}).  The videos' frames sit one after the other in one
 * buffer of L_total frames, their clips one after the other (video-major) in one clip list; evalutil.group_clip_table builds the tables, all DEVICE int32: seg_off[nv+1] first packed frame of
 * every video (seg_off[nv] = L_total), clip_off[nv+1] first clip of every video, starts[n] video-local first frame of
 * every clip, clip_base[n] / clip_len_v[n] = seg_off / length of the clip's video.  nv <= 65535.  max_len: the longest
 * video of the group (sizes grids, workgroups and LDS; a video longer than max_len is left out).  A table entry that
 * points outside the buffers it indexes is skipped, never followed. */
/* clips_out[b][t] = video[clip_base[b] + starts[b] + t] when 0 <= starts[b] + t < clip_len_v[b], else a zero frame: the
 * window is cut at the ends of the clip's OWN video.  Forms and limits of tdeed_clip_gather_u8. */
int tdeed_clip_gather_seg_u8(const uint8_t* video, int L_total, long frame_bytes, const int* starts, const int* clip_base,
                             const int* clip_len_v, int B, int T, uint8_t* clips_out, void* stream);
/* tdeed_clip_gather_seg_u8 over a VIRTUAL packed buffer of L_total frames of which only a ring of ring_frames rows is on the
 * device: packed frame p sits in ring[p % ring_frames] (the frame ring of a video longer than the device budget).  Which
 * frame a slot reads and whether it is padding is decided exactly as by _seg_u8 on the whole buffer.  That every frame a
 * clip reads is live in the ring when the launch runs (T <= ring_frames, upload order) is the caller's duty. */
int tdeed_clip_gather_ring_u8(const uint8_t* ring, int ring_frames, int L_total, long frame_bytes, const int* starts,
                              const int* clip_base, const int* clip_len_v, int B, int T, uint8_t* clips_out, void* stream);
/* Clip windows of per-frame ROWS: maps [rows][row_bytes] resident on the device (any element type; the trunk map of every
 * frame, computed once), of which the first L (L_total) rows are the frames of the video (the packed group).  out[b][t] =
 * maps[starts[b] + t] when that frame lies inside its video -- 0 <= starts[b] + t < L, or < clip_len_v[b] with the row offset
 * by clip_base[b] in the segmented form, exactly the windows of tdeed_clip_gather_u8 / _seg_u8 -- and maps[pad_row] otherwise
 * (the row of a black frame: its map is not zero).  L <= rows, 0 <= pad_row < rows.  16-byte accesses when row_bytes % 16 == 0
 * and both buffers are 16-byte aligned, a byte path otherwise.  B * T <= 65535. */
int tdeed_rows_gather(const void* maps, int rows, long row_bytes, int L, int pad_row, const int* starts, int B, int T, void* out,
                      void* stream);
int tdeed_rows_gather_seg(const void* maps, int rows, long row_bytes, int L_total, int pad_row, const int* starts,
                          const int* clip_base, const int* clip_len_v, int B, int T, void* out, void* stream);
/* clip_scores fp32 [V][n][T][K1] (V views of the n clips of the group's list).  Per packed frame p of video v (f = p -
 * seg_off[v]), over the clips i = clip_off[v] .. clip_off[v+1]-1 in the order given with 0 <= f - starts[i] < T, view after
 * view: track_sum[p] += clip_scores[view][i][f - starts[i]] and support[p] += 1 (count_all = 1: always; count_all = 0: only
 * when the added row has a non-zero entry).  track_sum [L_total][K1] and support int32[L_total] are accumulated onto (the
 * caller zeroes them); mean_out [L_total][K1] (or NULL) = track_sum / float(max(support, 1)).  One thread per frame, fixed
 * order, no atomics: per video bit-identical to the host loop of util/eval.py:284-349. */
int tdeed_stitch_scores_seg(const float* clip_scores, int V, int n, int T, int K1, const int* starts, const int* seg_off,
                            const int* clip_off, int nv, int count_all, int L_total, float* track_sum, int* support,
                            float* mean_out, void* stream);
/* tdeed_stitch_scores_seg for ONE video whose length is not known yet, one launch per batch of clips.  State between the
 * launches: ring_sum fp32 [ring_rows][K1] and ring_sup int32 [ring_rows], frame p in row p % ring_rows, zero before the
 * first launch.  clip_scores fp32 [V][B][T][K1]: the scores of this batch; starts: DEVICE int32[B], ascending, and ascending
 * over the launches.  Host scalars: lo = rows final before this launch, final_hi = rows final after it (no later clip covers
 * a frame below it), limit = frames that exist (frames at or beyond it are not touched).  One thread per frame p in [lo,
 * min(limit, max(final_hi, starts[B-1] + T))) adds the batch's clips onto its ring row as tdeed_stitch_scores_seg does (same
 * order, same support rule); for p < final_hi it writes out_sum[p - lo], out_sup[p - lo] and out_mean[p - lo] (or NULL) =
 * sum / float(max(support, 1)) and zeroes the ring row.  Over the launches of a stream the rows carry the bits of one
 * tdeed_stitch_scores_seg launch over the whole clip list.  The caller's duties: no clip of the batch covers a frame below lo,
 * and the frames of one launch fit the ring (ring_rows >= T + (B - 1) * (stride of the clip grid)).  B = 0 is legal (clip_scores
 * and starts may be NULL): it only writes out [lo, final_hi).  out_* may be NULL when final_hi == lo.  No atomics. */
int tdeed_stitch_live(const float* clip_scores, int V, int B, int T, int K1, const int* starts, int count_all, int lo,
                      int final_hi, int limit, int ring_rows, float* ring_sum, int* ring_sup, float* out_sum, int* out_sup,
                      float* out_mean, void* stream);
/* mean fp32 [L_total][K1] (tdeed_stitch_scores_seg's mean_out).  pred int32[L_total]: first maximum of each row (np.argmax),
 * pred_score fp32[L_total] that entry; pred_u8 (or NULL; K1 <= 256): pred in one byte per frame, the form in which it is
 * copied to the host.  Per video v and class c >= 1 the frames with mean[f][c] >= hr_threshold (fp32 comparison,
 * util/eval.py:160): count[v][c] += their number, first_frame[v][c] = min(first_frame[v][c], the first of them), in
 * video-local frames.  The caller fills row v of first_frame int32 [nv][K1] with the video's length and count int32 [nv][K1]
 * with 0. */
int tdeed_frame_events_seg(const float* mean, const int* seg_off, int nv, int L_total, int max_len, int K1, float hr_threshold,
                           int* pred, unsigned char* pred_u8, float* pred_score, int* first_frame, int* count, void* stream);
/* The frame error and foreground-F1 counters of util/eval.py:34-84 over a packed track: pred = the first maximum of each row of
 * mean fp32 [L_total][K1], true = labels uint8[L_total] (values < K1 <= 256).  stats int64 [2 + 3*K1] is ADDED to: frames,
 * frames with pred != true, then (tp, fp, fn) for "any" (foreground against background) and for every class k >= 1 at
 * 2 + 3*k.  Integer sums: the result does not depend on the order of accumulation. */
int tdeed_frame_stats_seg(const float* mean, const unsigned char* labels, int L_total, int K1, long* stats, void* stream);
/* bytes of workspace tdeed_nms_track_seg needs (0: max_len frames of suppression state fit the LDS of a workgroup) */
long tdeed_nms_track_seg_workspace(int L_total, int max_len, int K1);
/* threads of the suppression / compaction workgroups tdeed_nms_track_seg launches for this max_len */
int tdeed_nms_track_seg_threads(int max_len);
/* Exact hard (soft = 0, util/eval.py:195-226) or soft (soft = 1, util/eval.py:228-261) non-maximum suppression, per video,
 * of the high-recall candidates of every class c >= 1 (frames with mean[f][c] >= hr_threshold, score (double)mean[f][c]),
 * one workgroup per (class, video), in rounds (evalutil.nms_rounds states the rule); events are kept while their score is
 * >= threshold (double comparison).  windows: HOST int32[n_windows], n_windows = 1 (every class) or >= K1 - 1 (indexed by the
 * rank of (first_frame[v][c], c) among the classes of video v that have a candidate: the order in which labels appear in the
 * host's list); soft needs windows >= 1.  first_frame: DEVICE int32 [nv][K1] as tdeed_frame_events_seg leaves it.  emitted
 * uint8 [K1][L_total], kept_score double [K1][L_total], st_frame / st_class_u8 / st_score (L_total * (K1-1) entries each)
 * and st_count int32[nv] are scratch.  Output: the kept events of video v, ordered by ascending video-local frame and within
 * a frame by that rank (the host's stable sort), are entries event_off[v] .. event_off[v+1]-1 of out_frame (int32) /
 * out_class_u8 / out_score (double), each with room for L_total * (K1-1) entries: the videos' lists follow each other
 * densely in video order, event_off int32[nv+1].  rounds int32 [nv][K1]: rounds taken per class (<= its candidates).
 * Deterministic; K1 - 1 <= 64. */
int tdeed_nms_track_seg(const float* mean, const int* seg_off, int nv, int L_total, int max_len, int K1, float hr_threshold,
                        double threshold, int soft, const int* windows, int n_windows, const int* first_frame, void* workspace,
                        unsigned char* emitted, double* kept_score, int* st_frame, unsigned char* st_class_u8, double* st_score,
                        int* st_count, int* out_frame, unsigned char* out_class_u8, double* out_score, int* event_off, int* rounds,
                        void* stream);

/* ---- average precision of the spotted events (ap.hip) ----------------------------------------------------------------
 * The dataset: NV videos, video `ord` (the index of its name in sorted order) owns the frames vid_off[ord] .. vid_off[ord+1]-1
 * of LT_all (vid_off int32[NV+1]).  The truth: gt_off int32[NV*K1 + 1], entry ord*K1 + c the start of the ground-truth frames
 * of class c in video ord inside gt_frames int32[G], in the truth record's list order (duplicates stay).  All on the device. */
/* longest video whose events are ordered in LDS; longer ones are ordered in place in ev_score / ev_frame */
int tdeed_ap_lds_frames(void);
/* tolerances one launch takes */
int tdeed_ap_max_tolerances(void);
/* ground-truth frames one class may have in one video with n_tol tolerances (they live in LDS); 0: n_tol out of range */
int tdeed_ap_max_truth(int n_tol);
/* Segment + match, one workgroup per class c >= 1 and video v of a group's packed track (mean, seg_off, nv, L_total, max_len as
 * for tdeed_nms_track_seg; ords int32[nv] the videos' ordinals).  Events: emitted == NULL: the frames with mean[f][c] >=
 * hr_threshold, score (double)mean[f][c]; otherwise the frames with emitted[c][f] != 0, score kept_score[c][f], the planes
 * [K1][L_total] of tdeed_nms_track_seg.  They are ordered by score descending, frame ascending and stored: ev_score double /
 * ev_frame int32 [K1-1][LT_all] from vid_off[ord] on, ev_count int32 [K1-1][NV].  Then per tolerance (HOST int32[n_tol], each
 * >= 0) the greedy matching of util/score.py:45-96 restricted to the video: hit_pos int32 [n_tol][G], entry gt_off[ord*K1+c] + k
 * the position of the k-th hit in the ordered list, hit_count int32 [n_tol][NV*K1].  max_gt: the longest ground-truth list.
 * Deterministic: no atomics. */
int tdeed_ap_match_seg(const float* mean, const unsigned char* emitted, const double* kept_score, const int* seg_off, int nv,
                       int L_total, int max_len, int K1, float hr_threshold, const int* ords, int NV, const int* vid_off,
                       long LT_all, const int* gt_off, const int* gt_frames, int G, int max_gt, const int* tolerances, int n_tol,
                       double* ev_score, int* ev_frame, int* ev_count, int* hit_pos, int* hit_count, void* stream);
/* Rank + AP, once every video has been matched; the buffers above with a leading [n_entries] axis.  rank int32
 * [n_entries][n_tol][G]: per hit its 1-based position among all predictions of its class in the order score descending, video
 * ordinal ascending, frame ascending.  class_off int32[K1+1]: class c owns class_off[c] .. class_off[c+1]-1 of the G entries of
 * psorted double [n_entries][n_tol][G] (scratch; the precisions in rank order), i.e. class_off[c+1] - class_off[c] is the
 * class's ground-truth count.  ap double / nhits int32 [n_entries][n_tol][K1]: interpolated average precision and hits. */
int tdeed_ap_rank(const double* ev_score, const int* ev_count, const int* vid_off, int NV, long LT_all, const int* gt_off, int G,
                  int K1, int n_entries, int n_tol, const int* hit_pos, const int* hit_count, const int* class_off, int* rank,
                  double* psorted, double* ap, int* nhits, void* stream);
/* Exchange of the state between the ranks of a sharded pass.  ev_count / hit_count hold the sums over the ranks; sc_end int64
 * [n_entries*(K1-1)*NV] and hc_end int64 [n_entries*n_tol*NV*K1] are their inclusive scans in the stores' own order, so segment
 * s owns the elements end[s-1] .. end[s]-1 of a dense payload: scores double[n_scores], hits int32[n_hits] (the scans' last
 * entries).  own int32[NV]: non-zero for the videos this rank matched.  pack copies the used part of the own segments out of
 * ev_score / hit_pos (the buffers of tdeed_ap_rank) into the payloads, which the caller zeroes; unpack writes the segments of
 * the videos that are NOT own from the payloads into the stores and leaves own segments and ev_frame alone.  One thread per
 * payload element, a binary search in the scan; no atomics.  A payload may be NULL when it has no element. */
int tdeed_ap_state_pack(const double* ev_score, const int* hit_pos, double* scores, int* hits, const long* sc_end,
                        const long* hc_end, long n_scores, long n_hits, const int* own, const int* vid_off, const int* gt_off,
                        int NV, int K1, int n_entries, int n_tol, long LT_all, int G, void* stream);
int tdeed_ap_state_unpack(double* ev_score, int* hit_pos, const double* scores, const int* hits, const long* sc_end,
                          const long* hc_end, long n_scores, long n_hits, const int* own, const int* vid_off, const int* gt_off,
                          int NV, int K1, int n_entries, int n_tol, long LT_all, int G, void* stream);

/* ---- training clips drawn from resident videos (trainclips.hip) -----------------------------------------------------
 * frames: uint8 [total_frames][frame_bytes], the frames of all resident videos packed one after the other.  The tables are
 * DEVICE int64[B], per clip: first = first packed frame of the clip's video, nframes = that video's length, base = the
 * clip's first original frame (may be negative).  out[b][t] = frames[first[b] + base[b] + t*stride] when
 * 0 <= base[b] + t*stride < nframes[b], else a zero frame (FrameReader.load_paths / load_frames(pad=True),
 * dataset/frame.py:274-382): a window that hangs over the end of its video never reads the next one, and an entry that
 * points outside the packed buffer is not followed.  16-byte accesses when frame_bytes % 16 == 0 and both buffers are
 * 16-byte aligned, a byte path otherwise.  B * T <= 65535. */
int tdeed_train_clip_gather_u8(const uint8_t* frames, long total_frames, long frame_bytes, const long* first, const long* base,
                               const long* nframes, int B, int T, int stride, uint8_t* out, void* stream);
/* The same with one stride per clip: strides DEVICE int32[B], out[b][t] = frames[first[b] + base[b] + t*strides[b]] under the
 * same window rule, the same guards and the same two access widths (a joint batch mixes clips of sets sampled at different
 * strides).  The entry cannot read the table: the caller refuses an entry <= 0 on the host; the kernel does not follow one
 * (zero frames). */
int tdeed_train_clip_gather_u8_ps(const uint8_t* frames, long total_frames, long frame_bytes, const long* first, const long* base,
                                  const long* nframes, int B, int T, const int* strides, uint8_t* out, void* stream);
/* Mixup of two such windows without their uint8 intermediates: out fp32 [B][T][frame_bytes] =
 * lam[b] * A[b][t] + (1 - lam[b]) * B[b][t], bit for bit what tdeed_mix_frames gives on the two batches
 * tdeed_train_clip_gather_u8 would write (a padded frame contributes 0).  4-byte loads / 16-byte stores when
 * frame_bytes % 4 == 0 and the buffers are aligned for them, a scalar path otherwise. */
int tdeed_train_clip_gather_mix_f32(const uint8_t* frames, long total_frames, long frame_bytes, const long* first_a,
                                    const long* base_a, const long* nframes_a, const long* first_b, const long* base_b,
                                    const long* nframes_b, const float* lam, int B, int T, int stride, float* out, void* stream);
/* The same with one stride per clip, shared by its two operands: strides DEVICE int32[B]; bit for bit tdeed_mix_frames on the
 * two batches tdeed_train_clip_gather_u8_ps would write.  The same 4-byte load / 16-byte store path and scalar path. */
int tdeed_train_clip_gather_mix_f32_ps(const uint8_t* frames, long total_frames, long frame_bytes, const long* first_a,
                                       const long* base_a, const long* nframes_a, const long* first_b, const long* base_b,
                                       const long* nframes_b, const float* lam, int B, int T, const int* strides, float* out,
                                       void* stream);
/* Labels of n clips (dataset/frame.py:151-159, 226-233): clip_video / clip_base DEVICE int64[n] (video index, first original
 * frame), ev_off int32[nv+1] / ev_frame / ev_class int32[n_events] the videos' events in file order.  Per (clip, t) the
 * events of the clip's video are walked in order, idx = floor((ev_frame - base) / stride); the last one with
 * |t - idx| <= r gives label[clip][t] = its class and labelD[clip][t] = t - idx, 0 / 0 when there is none.  label / labelD
 * int64 [n][T] (labelD may be NULL).  One thread per position, no atomics. */
int tdeed_clip_labels(const long* clip_video, const long* clip_base, int n, int T, int stride, int r, const int* ev_off,
                      const int* ev_frame, const int* ev_class, int nv, int n_events, long* label, long* labelD, void* stream);
/* The same with one stride per clip: strides DEVICE int32[n], idx = floor((ev_frame - base) / strides[clip]).  A clip whose
 * entry is <= 0 gets 0 / 0 everywhere (the caller refuses such a table on the host). */
int tdeed_clip_labels_ps(const long* clip_video, const long* clip_base, int n, int T, const int* strides, int r, const int* ev_off,
                         const int* ev_frame, const int* ev_class, int nv, int n_events, long* label, long* labelD, void* stream);

/* ---- backward of the SGP encoder-decoder (training path; sgp_bwd.hip) ------------------------------------------
 * Activations and activation gradients share the forward dtype; parameter gradients are fp32.  Every parameter
 * gradient is produced as caller-owned per-workgroup partials (`part*`) folded in a fixed order: no float atomics,
 * a step is bit-reproducible. */
/* out[j] (+)= sum_p part[p][j], p < P, j < n */
int tdeed_reduce_partials(const float* part, int P, long n, float* out, int accumulate, void* stream);
/* the same over rows that are `stride` floats apart (several parameter groups side by side in one partial row) */
int tdeed_reduce_strided(const float* part, int P, long stride, long n, float* out, void* stream);
/* gradient write-out of a whole step in one launch: tab = device array of nt records {const float* src; long dst_offset;
 * long n; long first_chunk} (first_chunk = running sum of ceil(n / 4096) over the records before it), n_chunks = that sum
 * over all records; dst[off + i] = (accumulate ? dst[off + i] : 0) + scale * src[i]. */
int tdeed_multi_copy(const void* tab, int nt, long n_chunks, float* dst, float scale, int accumulate, void* stream);
/* the same write-out with the fold of per-workgroup partials inside.  tab: device array of nt entries of 8 int64
 * {src pointer, dst offset, n, first workgroup, P | cw << 32, pstride, cols, ld}: P == 1 copies n elements from a source of
 * `cols` contiguous elements per row, rows `ld` apart (4096 elements per workgroup); P > 1 writes
 * dst[off + j] = scale * sum_p src[p * pstride + j] with cw = tdeed_multi_fold_cw(P, n) columns per workgroup (the partials
 * tdeed_wgrad leaves when called with accumulate = -1).  n_wgs = total workgroups of all entries. */
int tdeed_multi_fold_cw(int P, long n);
int tdeed_multi_fold(const void* tab, int nt, long n_wgs, float* dst, float scale, int accumulate, void* stream);
/* mode 0: y = gelu(x); 1: y = dy * gelu'(x); 2: y = x + dy; 3: y = x * dy.  n elements, multiple of 8 */
int tdeed_eltwise(const void* x, const void* dy, void* y, long n, int mode, int dtype, void* stream);
/* [R][Cc] -> [Cc][R] (weight transposes for the input-gradient contractions) */
int tdeed_transpose(const void* x, int R, int Cc, void* y, int dtype, void* stream);
/* weight / bias gradient of a Conv1d(k=1) / 1x1 conv: dW[n][k] (+)= sum_m dY[m][n] X[m][k], db[n] (+)= sum_m dY[m][n]
 * (db may be NULL).  part_w fp32 [Z][N][K], part_b fp32 [Z][N], Z = tdeed_wgrad_slices(M, N, K).
 * accumulate = -1: the partials are left unfolded (dW / db may be NULL; part_b is filled when given): tdeed_multi_fold folds
 * them together with the gradient write-out. */
int tdeed_wgrad_slices(int M, int N, int K);
/* X0 (optional, bf16, M >= 4096): columns k < k0 of the X operand come from X0 (row stride ldx0): the gate-shift splice
 * [G | x[:, k0:]] of a conv1 operand is never materialised (as A0 / k0 of tdeed_gemm_fwd) */
int tdeed_wgrad(const void* dY, long ldy, const void* X, long ldx, const void* X0, long ldx0, int k0, int M, int N, int K,
                float* part_w, float* part_b, float* dW, float* db, int accumulate, int dtype, void* stream);
/* channel LayerNorm backward (modules.py:320-363): dx (+)= d/dx, dw/db [C].  part fp32 [tdeed_layernorm_bwd_blocks(rows)][2][C] */
int tdeed_layernorm_bwd_blocks(int rows);
int tdeed_layernorm_bwd(const void* x, long ldx, const void* dy, long ldy, int rows, int C, const float* w, float eps,
                        void* dx, int accumulate, float* part, float* dw, float* db, int dtype, void* stream);
/* GroupNorm(G) backward over NTC slabs.  part fp32 [B][2][C] */
int tdeed_groupnorm_bwd(const void* x, const void* dy, int B, int T, int C, int G, const float* w, float eps, void* dx,
                        int accumulate, float* part, float* dw, float* db, int dtype, void* stream);
/* depthwise-branch backward of SGPBlock (modules.py:164-170) and of either input of SGPMixer (modules.py:290-305):
 * o = branch input (row stride ldo); g_conv / g_inst / g_id = gradients of (convw+convkw)*psi, of fc*phi and of the
 * identity term (row stride ldg; SGPBlock passes one tensor three times, SGPMixer three slabs of d cat); d_o (row
 * stride ld_do); d_dw [C][2ks+up+2], d_db [5][C] in tdeed_sgp_branch_fwd's packed layouts.
 * part_w fp32 [B][C][2ks+up+2], part_b fp32 [B][5][C]. */
int tdeed_sgp_branch_bwd(const void* o, long ldo, const void* g_conv, const void* g_inst, const void* g_id, long ldg,
                         int B, int T, int C, int ks, int up, const float* dw, const float* db, void* d_o, long ld_do,
                         float* part_w, float* part_b, float* d_dw, float* d_db, int dtype, void* stream);
/* nn.Upsample(linear, align_corners=True) backward: d_xu [B][T_hi][.] (row stride ld) -> d_xn [B][T_lo][C] */
int tdeed_upsample_bwd(const void* d_xu, long ld, int B, int T_hi, int T_lo, int C, void* d_xn, int dtype, void* stream);
/* nn.AdaptiveMaxPool1d backward (first maximum of a window takes the gradient, like torch) */
int tdeed_maxpool_bwd(const void* x, const void* dy, int B, int T_in, int T_out, int C, void* dx, int dtype,
                      void* stream);


/* ---- train-mode trunk pieces (trunk_bwd.hip): BatchNorm with batch statistics, SE with kept intermediates, grouped
 * 3x3 backward.  Maps are channels-last [M][C] in the activation dtype; statistics and parameter gradients fp32. */
int tdeed_bn_slabs(long M);
/* statistics of the raw conv map z: mean/rstd (kept for the backward), a = w*rstd, b = bias - mean*a (for
 * tdeed_bn_apply), running_mean/var updated in place when non-NULL (momentum 0.1, unbiased variance, like
 * nn.BatchNorm2d).  part fp32 [tdeed_bn_slabs(M)][2][C] */
int tdeed_bn_train_stats(const void* z, long M, int C, const float* w, const float* bias, float eps, float momentum,
                         float* part, float* mean, float* rstd, float* a, float* b, float* run_mean, float* run_var,
                         int dtype, void* stream);
/* the finalisation alone, from partial sums a producer's epilogue wrote (see tdeed_gemm_fwd colpart, tdeed_gconv3x3_fwd
 * pooled_sq): P rows of per-channel sums (part_s) / sums of squares (part_q), pstride floats apart, covering M rows */
int tdeed_bn_finalize(const float* part_s, const float* part_q, long pstride, int P, long M, int C, const float* w,
                      const float* bias, float eps, float momentum, float* mean, float* rstd, float* a, float* b,
                      float* run_mean, float* run_var, void* stream);
/* out[s][j] = sum of part[p * pstride + j] over the rows p of slice s (slices of ceil(P / slices) rows), j < n; rows of out
 * are `ostride` floats apart.  A first fold for tdeed_bn_finalize when a producer left one partial row per (frame, band). */
int tdeed_fold_rows(const float* part, long pstride, int P, int n, int slices, float* out, long ostride, void* stream);
/* y = act(z * a[c] + b[c] + res) */
int tdeed_bn_apply(const void* z, long M, int C, const float* a, const float* b, const void* res, int relu, void* y,
                   int dtype, void* stream);
/* y = act(z * a + b + (res * ra + rb)): the same with the residual a raw conv output under its own BatchNorm affine (the
 * shortcut conv of a downsampling bottleneck: its normalised map is never written) */
int tdeed_bn_apply2(const void* z, long M, int C, const float* a, const float* b, const void* res, const float* ra,
                    const float* rb, int relu, void* y, int dtype, void* stream);
/* ... and y2 [M][Fp2]: a compact copy of output channels [0, F2) (zeros in [F2, Fp2)) -- the dense slice the next block's
 * gate-shift module reads (what tdeed_gsf_slice would make with a pass of its own); ra / rb may be NULL */
int tdeed_bn_apply_slice(const void* z, long M, int C, const float* a, const float* b, const void* res, const float* ra,
                         const float* rb, int relu, void* y, void* y2, int F2, int Fp2, int dtype, void* stream);
/* BatchNorm (training) backward; when relu != 0 the ReLU mask comes from y (the block's output) or, with y NULL (no
 * residual in front of the ReLU), from z through the forward affine fa, fb (y > 0 <=> fa*z + fb > 0: one map less to
 * read); d_res (optional) receives the masked gradient = gradient of the residual summed in before the ReLU.  sums fp32
 * [2][C]: sums[0] = db, sums[1] = dw (also copied to db / dw when those are non-NULL). */
int tdeed_bn_train_bwd(const void* z, const void* dy, const void* y, int relu, long M, int C, const float* mean,
                       const float* rstd, const float* w, const float* fa, const float* fb, float* part, float* sums,
                       void* dz, void* d_res, float* dw, float* db, int dtype, void* stream);
/* p[n][c] = mean_px x (x2 NULL: the SE squeeze) or sum_px x*x2 (gradient of the SE gate).  aff_on = 1 / 2: x / x2 is a
 * raw conv output and relu(in_a[c] * . + in_b[c]) (BatchNorm + ReLU) is applied on load; 0: none (in_a, in_b may be NULL) */
int tdeed_pool_rows(const void* x, const void* x2, int N, int hw, int C, const float* in_a, const float* in_b, int aff_on,
                    float* p, int dtype, void* stream);
/* SE excitation keeping the hidden units: w1t [C][R], w2t [R][C] */
int tdeed_se_train_fwd(const float* p, int N, int C, int R, const float* w1t, const float* b1, const float* w2t,
                       const float* b2, float* hid, float* gate, void* stream);
/* its backward: w1 [R][C], w2 [C][R]; d_pre2 [N][C], d_hid [N][R] feed tdeed_wgrad, d_p [N][C] is d(squeeze) */
int tdeed_se_train_bwd(const float* d_gate, const float* gate, const float* hid, int N, int C, int R, const float* w1,
                       const float* w2, float* d_pre2, float* d_hid, float* d_p, void* stream);
/* y[n][px][c] = x'[n][px][c] * s[n][c] + add[n][c] * add_scale (add may be NULL); x' = x, or with in_a / in_b given
 * relu(in_a[c] * x + in_b[c]) (x a raw conv output: BatchNorm + ReLU applied on load) */
int tdeed_scale_rows(const void* x, const float* s, const float* add, float add_scale, int N, int hw, int C,
                     const float* in_a, const float* in_b, void* y, int dtype, void* stream);
/* conv1's BatchNorm backward with the statistics from conv2's input-gradient launch (stride-1 bottlenecks, bf16):
 *   tdeed_gconv3x3_dgrad_stats: dx [N][Hi][Wi][C] = grouped 3x3 conv of dy with the flipped / transposed weights (wfrag_t,
 *     packed like tdeed_gconv3x3_fwd's wfrag; one / zero: fp32 [C] ones / zeros), and part_s / part_q fp32
 *     [N][tdeed_gconv3x3_parts(Hi, Wi, C, 1)][C]: per (frame, band) sums of g and g * (bz - bmean), g = dx * [bfa bz + bfb > 0]
 *     (bz: conv1's raw output, bfa / bfb its BatchNorm affine, bmean its batch mean);
 *   tdeed_bn_bwd_masked_from_parts: folds such partial rows (P rows, pstride floats apart) into sums fp32 [2][C]
 *     (d bias, d weight) and runs the apply pass dz = k1 g + k2 z + k3 with the ReLU mask recomputed from z. */
int tdeed_gconv3x3_dgrad_stats(const void* dy, int N, int Hi, int Wi, int C, int gw, const void* wfrag_t, const float* one,
                               const float* zero, void* dx, const void* bz, const float* bfa, const float* bfb,
                               const float* bmean, float* part_s, float* part_q, void* stream);
/* stride-2 blocks: tdeed_gconv3x3_bwd (stride 2, bf16) whose input-gradient launch leaves the same partial rows:
 * part_s / part_q fp32 [N * tdeed_gconv3x3_bwd_stats_bands(Hi)][C] */
int tdeed_gconv3x3_bwd_stats_bands(int Hi);
int tdeed_gconv3x3_bwd_stats_fits(int N, int Hi, int Wi, int C, int gw);
int tdeed_gconv3x3_bwd_stats(const void* x, const void* dy, int N, int Hi, int Wi, int C, int gw, const float* w,
                             const float* in_a, const float* in_b, void* dx, float* part, float* dw, const void* bz,
                             const float* bfa, const float* bfb, const float* bmean, float* part_s, float* part_q, void* stream);
int tdeed_bn_bwd_masked_from_parts(const void* z, const void* dy, long M, int C, const float* mean, const float* rstd,
                                   const float* w, const float* fa, const float* fb, const float* part_s, const float* part_q,
                                   long pstride, int P, float* sums, void* dz, int dtype, void* stream);
/* conv1 backward of a NARROW training bottleneck in one launch (csrc/trunk_bwd3.hip; bf16; (Co, Ci) = (64, 32), (128, 64),
 * (128, 128), (64, 64): RegNetY-800MF s1 / s2; with fa = 0, fb = 1 and no R / sink also conv3's backward there): from conv2's input gradient dY and conv1's raw output Z ([M][Co]) the BatchNorm + ReLU
 * backward dz1 (never stored), the input gradient dX [M][Ci] = dz1 @ W1 + shortcut gradient, masked by [X > 0] with the
 * gradient sink's column sums (as tdeed_gemm_dgrad), and the partial weight gradients dz1^T @ X.
 * fa / fb / mean / rstd / w: conv1's BatchNorm; sums fp32 [2][Co] = (sum g, sum g xhat) of its backward; Wt [Ci][Co] = W1^T;
 * R: shortcut gradient [M][Ci] (r_hi > 0: rows of the even pixels of an r_hi x r_wi frame) or NULL; bpart fp32
 * [grid][3][Ci] (or NULL), wpart fp32 [grid][Co][Ci], grid = tdeed_narrow_conv1_bwd_grid(M, Co, Ci).
 * Z == NULL (not at 128 <- 128): Z is X @ W1^T of exactly these operands and is recomputed in the launch instead of read. */
int tdeed_narrow_conv1_bwd_fits(int Co, int Ci);
int tdeed_narrow_conv1_bwd_grid(long M, int Co, int Ci);
int tdeed_narrow_conv1_bwd(const void* dY, const void* Z, long M, int Co, int Ci, const float* fa, const float* fb,
                           const float* mean, const float* rstd, const float* w, const float* sums, const void* X, const void* Wt,
                           const void* R, long ldr, int r_hi, int r_wi, void* dX, int use_mask, const void* bz,
                           const float* bmean, const void* bzd, const float* bmean_d, float* bpart, float* wpart, void* stream);
/* sums fp32 [2][C] = (sum_p part_s, rstd * sum_p part_q) over P partial rows pstride floats apart (what
 * tdeed_gconv3x3_dgrad_stats / tdeed_gconv3x3_bwd_stats leave) */
int tdeed_bn_sums_from_parts(const float* part_s, const float* part_q, long pstride, int P, int C, const float* rstd,
                             float* sums, void* stream);
/* SE + conv2-BatchNorm backward of a bottleneck without the d_y2 map (csrc/trunk_bwd2.hip; timm SEModule / BatchNorm2d under
 * autograd, /root/reference/model/model.py:265-324).  d = d(y2 * gate) [N][hw][C] (conv3's input gradient), z = conv2's raw
 * output, y2 = relu(fa * z + fb):
 *   tdeed_se_bn_bwd_sums:     sums fp32 [5][N][C] = per (frame, channel) sum over the pixels of
 *                             d*y2 | d*m | d*m*(z-mean) | m | m*(z-mean),  m = [fa z + fb > 0];  sums[0] is d(gate)
 *   tdeed_se_bn_bwd_finalize: out fp32 [2][C] = (sum g, sum g * xhat) with g = m * (d * gate + d_p / hw): the conv2
 *                             BatchNorm's (d bias, d weight), from the frame sums, gate [N][C] and d_p [N][C] = d(squeeze)
 *   tdeed_se_bn_bwd_apply:    dz [N][hw][C] = k1 * g + k2 * z + k3 (the BatchNorm input gradient), g formed on the fly */
int tdeed_se_bn_bwd_sums(const void* d, const void* z, int N, int hw, int C, const float* fa, const float* fb,
                         const float* mean, float* sums, int dtype, void* stream);
int tdeed_se_bn_bwd_finalize(const float* sums, const float* gate, const float* d_p, int N, int hw, int C, const float* rstd,
                             float* out, void* stream);
int tdeed_se_bn_bwd_apply(const void* d, const void* z, const float* gate, const float* d_p, int N, int hw, int C,
                          const float* fa, const float* fb, const float* mean, const float* rstd, const float* w,
                          const float* sums, void* dz, int dtype, void* stream);
/* "Gradient sink" (csrc/trunk_bwd2.hip, gemm.hip): the ReLU backward at a block's output and the statistics pass of the
 * BatchNorm backward behind it, applied by the kernels that PRODUCE the gradient (timm Bottleneck under autograd,
 * /root/reference/model/model.py:265-324).
 * tdeed_gemm_dgrad: C [M][N] = ((A [M][K] @ W [N][K]^T) + R) * [mask > 0]; with r_hi > 0 the residual R has rows only for the
 *   even pixels of an r_hi x r_wi frame (stride-2 shortcut); C2 (optional, [M][n2]) takes columns [0, n2) BEFORE the residual
 *   and C keeps only the residual there (gate-shift blocks); bpart (optional) fp32 [ceil(M/128)][3][N]: per-tile column sums of
 *   the stored v, v * (bz - bmean) and (bzd given) v * (bzd - bmean_d).
 * tdeed_gsf_add_cols_sink: dx[m][c] += (a + b)[m][c] * [mask > 0] for c < Fp, with the sums of what was ADDED in
 *   part fp32 [tdeed_gsf_add_cols_sink_parts(M, Fp, dtype)][3][Fp] (mask / part may be NULL).
 * tdeed_bn_bwd_from_parts: BatchNorm backward of z [M][C] for an already masked gradient g whose column sums lie in producer
 *   partials: partA PA rows of [3][C] (+ partB PB rows of [3][nB] for columns [0, nB)); q = 1 / 2 selects the product row;
 *   sums fp32 [2][C] = (d bias, d weight); dz (may be NULL) = the input gradient; tmp fp32 [2 * 64 * 3 * C]. */
int tdeed_gemm_dgrad(const void* A, long lda, int M, int K, int N, const void* W, long ldw, const void* R, long ldr, int r_hi,
                     int r_wi, void* C, long ldc, void* C2, long ldc2, int n2, const void* mask, long ldmask, const void* bz,
                     long ldbz, const float* bmean, const void* bzd, long ldbzd, const float* bmean_d, float* bpart, int dtype,
                     void* stream);
/* tdeed_gemm_dgrad for K = N = 320 over many rows on the register-stationary contraction (Wfrag = the packed [N][K] matrix,
 * packing.pack_ws_weights): residual and mask required, no stride-2 residual, no second statistics map;
 * bpart fp32 [tdeed_gemm_rs_grid(M)][3][N]. */
int tdeed_gemm_dgrad_rs(const void* A, long lda, int M, int K, int N, const void* Wfrag, const void* R, long ldr, void* C,
                        long ldc, void* C2, long ldc2, int n2, const void* mask, long ldmask, const void* bz, long ldbz,
                        const float* bmean, float* bpart, void* stream);
int tdeed_gsf_add_cols_sink_parts(long M, int Fp, int dtype);
int tdeed_gsf_add_cols_sink(const void* a, const void* b, long M, int C, int Fp, void* dx, const void* mask, long ldmask,
                            const void* bz, long ldbz, const float* bmean, const void* bzd, long ldbzd, const float* bmean_d,
                            float* part, int dtype, void* stream);
/* tdeed_gsf_add_cols_sink with the backward of the module's BatchNorm3d applied to b on load: b = the gradient at the
 * BatchNorm's output (d_bn of tdeed_gsf_bwd), bnx [M][Fp] its input (the dense slice), bn_sums fp32 [2][Fp] = (sum g,
 * sum g xhat) as tdeed_bn_bwd_from_parts leaves them, bn_mean / bn_rstd / bn_w [Fp]: batch statistics and weight
 * (torch.nn.BatchNorm3d under autograd, /root/reference/model/impl/gsf.py:38-93). */
int tdeed_gsf_add_cols_sink_bn(const void* a, const void* b, long M, int C, int Fp, void* dx, const void* mask, long ldmask,
                               const void* bz, long ldbz, const float* bmean, const void* bzd, long ldbzd,
                               const float* bmean_d, float* part, const void* bnx, const float* bn_sums, const float* bn_mean,
                               const float* bn_rstd, const float* bn_w, int dtype, void* stream);
int tdeed_bn_bwd_from_parts(const void* z, const void* g, long M, int C, const float* mean, const float* rstd, const float* w,
                            const float* partA, int PA, const float* partB, int PB, int nB, int q, float* tmp, float* sums,
                            void* dz, int dtype, void* stream);
/* grouped 3x3 backward: dx (may be NULL: a stride-1 input gradient is itself a grouped 3x3 conv of dy with the flipped,
 * transposed weights and can run on tdeed_gconv3x3_fwd's MFMA kernel) and dw (fp32, the forward's packed [G][9][gw][gw]).
 * part fp32 [tdeed_gconv_wgrad_slabs(N*Ho*Wo)][G*9*gw*gw] */
int tdeed_gconv_wgrad_slabs(long npix_out);
/* in_a, in_b (optional, bf16): x is the raw output of the conv in front, relu(in_a[c] * x + in_b[c]) is applied on load
 * (as in tdeed_gconv3x3_fwd) */
int tdeed_gconv3x3_bwd(const void* x, const void* dy, int N, int Hi, int Wi, int C, int gw, int stride, const float* w,
                       const float* in_a, const float* in_b, void* dx, float* part, float* dw, int dtype, void* stream);
/* mode 0: out[(f,yo,xo)] = in[(f,2yo,2xo)] (operand of the stride-2 shortcut conv); mode 1: out[(f,2yo,2xo)] += in[(f,yo,xo)] */
int tdeed_stride2_rows(const void* in, void* out, int F, int hi, int wi, int C, int mode, int dtype, void* stream);

/* avgpool + positional encoding backward: d x[f][p][c] = d feat[f][c]/hw, d temp_enc[t][c] = sum_b d feat[b][t][c] */
int tdeed_avgpool_posenc_bwd(const void* d_feat, int B, int T, int hw, int C, void* dx, float* d_temp_enc, int dtype,
                             void* stream);
/* stem weight gradient (the uint8 input needs none): dz [N][Ho][Wo][32] -> dw [32][3][3][3]; part fp32
 * [N * ceil(Ho/16)][864] */
int tdeed_stem_wgrad(const void* frames, int frames_f32, int N, int H, int W, int crop_top, int crop_left, int crop_h, int crop_w,
                     int flip, const unsigned char* flip_mask /* NULL or [N], as tdeed_stem_fwd */, const void* dz,
                     float* part, float* dw, int dtype, void* stream);
/* tdeed_stem_wgrad with the stem BatchNorm's backward (torch.nn.BatchNorm2d of timm's stem ConvNormAct under autograd) applied
 * while the gradient rows are staged: g = the masked gradient at the BatchNorm's output, z = the raw stem output, sums fp32
 * [2][32] = (sum g, sum g xhat) as tdeed_bn_bwd_from_parts leaves them, mean / rstd / w [32].  bf16; geometry per
 * tdeed_stem_wgrad_bn_fits. */
int tdeed_stem_wgrad_bn_fits(int H, int W, int crop_h, int crop_w);
int tdeed_stem_wgrad_bn(const void* frames, int frames_f32, int N, int H, int W, int crop_top, int crop_left, int crop_h,
                        int crop_w, int flip, const unsigned char* flip_mask, const void* g, const void* z, const float* sums,
                        const float* mean, const float* rstd, const float* w, float* part, float* dw, void* stream);

/* train-time augmentation inside Impl.forward (model.py:76-83, 154-157): per clip ColorJitter(hue), (saturation),
 * (brightness), (contrast), GaussianBlur(5) on the cropped frames (torchvision 0.18.1 float-tensor arithmetic restated in
 * csrc/augment.hip); RandomHorizontalFlip is the flip_mask of tdeed_stem_fwd.  prm fp32 [B][8] on the device =
 * {hue shift, saturation, brightness, contrast, blur sigma (0 = off), -, -, -}, identity = {0,1,1,1,0}.  frames uint8 (or
 * fp32 0..255) [B*T][3][H][W] -> out fp32 0..255 [B*T][3][crop_h][crop_w] (feed to tdeed_stem_fwd with frames_f32 = 1 and
 * no crop).  part: tdeed_augment_scratch_floats(B*T) floats; tmp: same size as out (blur staging). */
long tdeed_augment_scratch_floats(int N);
int tdeed_augment_clips(const void* frames, int frames_f32, int B, int T, int H, int W, int crop_top, int crop_left,
                        int crop_h, int crop_w, const float* prm, float* part, float* out, float* tmp, void* stream);

/* mixup (model.py:240-256): out[b] = lam[b]*a[b] + (1-lam[b])*b[b], uint8 clips -> fp32 frames for tdeed_stem_fwd(frames_f32=1) */
int tdeed_mix_frames(const uint8_t* a, const uint8_t* b, const float* lam, int B, long per_clip, float* out, void* stream);

/* ---- gate-shift-fuse backward (gsf_bwd.hip; forward tensors as saved by tdeed_gsf_gate_fwd / tdeed_gsf_weight_fwd).
 * tdeed_gsf_slice: dense copy xs [M][Fp] of the module's channels (cols >= F zero): the BatchNorm3d operand in training.
 * tdeed_gsf_bwd: from dA (gradient of the module output in conv1's operand layout, [N*hw][Fp]) to d_xs (direct part of
 *   d x, dense [M][Fp]) and d_bn (gradient at the BatchNorm3d output, ReLU mask applied, dense [M][Fp]); parameter
 *   gradients d_w3 [F][27] (conv3D.weight flattened), d_b3 [2], d_cw [2][18] (channel_conv1 | channel_conv2), d_cb [2].
 *   w3 = conv3D.weight as [F][27]; sa/sb = the BatchNorm3d affine of this step; scratch fp32
 *   [tdeed_gsf_bwd_scratch_floats(B,T,hw,F)].
 * tdeed_gsf_add_cols: dx[m][0:Fp] += a[m][:] + b[m][:] (dx row stride C). */
int tdeed_gsf_slice(const void* x, long M, int C, int F, int Fp, void* xs, int dtype, void* stream);
long tdeed_gsf_bwd_scratch_floats(int B, int T, int hw, int F);
/* tdeed_gsf_bwd_part_layout: where tdeed_gsf_bwd(d_w3 == NULL) leaves its parameter-gradient partials inside `scratch`
 *   (float offsets): out[6] = {off_cw, rows_cw, stride_cw, off_w3, rows_w3, stride_w3}; part_cw row columns 0..17
 *   channel_conv1 taps, 18 its bias, 19..36 channel_conv2 taps, 37 its bias; part_w3 row = conv3D.weight [F][27], 2 biases
 *   (replaces nothing in the reference: autograd accumulates these in model/impl/gsf.py:38-93's backward). */
int tdeed_gsf_bwd_part_layout(int B, int T, int hw, int F, long* out);
int tdeed_gsf_bwd(const void* x, const float* gate, const float* fw, const float* ysum, const float* xsum,
                  const void* dA, int B, int T, int h, int w, int C, int F, int Fp, const float* w3, const float* sa,
                  const float* sb, const float* cw1, const float* cw2, float* scratch, void* d_xs, void* d_bn,
                  float* d_w3, float* d_b3, float* d_cw, float* d_cb, int dtype, void* stream);
int tdeed_gsf_add_cols(const void* a, const void* b, long M, int C, int Fp, void* dx, int dtype, void* stream);
/* tdeed_gsf_bwd that also leaves the statistics of the module's BatchNorm3d backward: bn_part fp32
 * [tdeed_gsf_bwd_bn_parts(B,T,h,w,C,Fp)][3][Fp], rows 0 / 1 = per-workgroup sums of d_bn and d_bn * (x - bn_mean) (the layout
 * tdeed_bn_bwd_from_parts folds with q = 1); tdeed_gsf_bwd_bn_parts == 0: not served at this geometry.  In both entries
 * d_w3 == NULL leaves the parameter gradients as partials inside scratch (layout in gsf_bwd.hip) for the caller's fold. */
int tdeed_gsf_bwd_bn_parts(int B, int T, int h, int w, int C, int Fp);
int tdeed_gsf_bwd_stats(const void* x, const float* gate, const float* fw, const float* ysum, const float* xsum,
                        const void* dA, int B, int T, int h, int w, int C, int F, int Fp, const float* w3, const float* sa,
                        const float* sb, const float* cw1, const float* cw2, float* scratch, void* d_xs, void* d_bn,
                        float* d_w3, float* d_b3, float* d_cw, float* d_cb, const float* bn_mean, float* bn_part, int dtype,
                        void* stream);

/* ---- data-parallel gradient reduction over RCCL / xGMI (comm.hip) ---------------------------------------------------
 * New functionality (the reference is single-GPU: model/model.py:184-190): one process per GPU, one
 * communicator with its own high-priority HIP stream.  tdeed_comm_all_reduce enqueues an in-place SUM of buf[0,n) over all
 * ranks behind the work already given to `compute_stream` and returns at once (the backward goes on); tdeed_comm_join makes
 * `compute_stream` wait for every collective enqueued so far (call it before the optimizer reads the gradients; the 1/world
 * goes into tdeed_adamw_step's grad_scale).  No host synchronisation in either; legal under stream capture.  librccl is
 * dlopen'ed at the first tdeed_comm_* call.  id128: 128 opaque bytes made on rank 0 (tdeed_comm_unique_id) and handed to
 * every rank by the caller (torch.distributed broadcast, a file ...); tdeed_comm_init is collective over the ranks. */
int tdeed_comm_unique_id(void* id128);
int tdeed_comm_init(void** comm_out, const void* id128, int world, int rank);
int tdeed_comm_info(void* comm, int* world, int* rank);
int tdeed_comm_all_reduce(void* comm, void* buf, long n, int dtype, void* compute_stream);
/* the same sum as reduce-scatter + all-gather over the first floor(n / world) * world elements plus a plain all-reduce of the
 * (< world) elements behind them: for the large bucket on point-to-point xGMI; any n is legal */
int tdeed_comm_all_reduce_rs_ag(void* comm, void* buf, long n, int dtype, void* compute_stream);
int tdeed_comm_join(void* comm, void* compute_stream);
int tdeed_comm_destroy(void* comm);

/* ---- HIP graph capture of a launch sequence (replaces eager op-by-op dispatch) ---------------
 * begin: hipStreamBeginCapture(stream); end: EndCapture + Instantiate -> handle; launch replays. */
int tdeed_graph_begin(void* stream);
int tdeed_graph_end(void* stream, void** graph_exec);
int tdeed_graph_launch(void* graph_exec, void* stream);
int tdeed_graph_destroy(void* graph_exec);

/* ---- dense contractions of the SGP encoder-decoder with their prologue / epilogue (csrc/sgp_gemm.hip; round 5).
 * Replaces, per SGPBlock / SGPMixer of /root/reference/model/modules.py: self.gn + self.mlp[0] + GELU (134-138, 186, 316),
 * self.mlp[2] + the residual add (186, 316) with the AdaptiveMaxPool1d of the encoder (64, 75-77) and the row sums the next
 * LayerNorm needs (320-363), concat_fc + GELU (245-246, 307-308) with the channel sums the next GroupNorm needs.
 * Weights: MFMA fragments [N/16][tdeed_sgp_gemm_ksteps(K)][64][8] bf16 (zero padded).  Row tiles never straddle clips.
 *   form = 16 * MT + NT (tile = 16 MT rows x 64 NT features) from tdeed_sgp_gemm_form; tdeed_sgp_gemm_row_tiles(T, MT) row
 *   tiles per clip (NJ), tdeed_sgp_gemm_col_tiles(N, NT) column tiles (nct).
 * tdeed_sgp_gemm_gn_gelu:   H[B*T][N] bf16 = GELU(GroupNorm_G(y) . W^T + b); y [B*T][K] in dtype_a; chsum [parts][B][K][2]
 *   (sum, sum of squares over the clip's rows per channel, summed over `parts` in order).
 * tdeed_sgp_gemm_residual:  out = resid + H . W^T + b (H bf16 [B*T][K]; out, resid, pooled in dtype_o); rowstat_part
 *   [nct][B*T][2] = (sum, sum of squares) of each stored row over the column tile; pooled != NULL (needs T == 2 T_out):
 *   the max of each row pair [B*T_out][N] and rowstat_pool_part [nct][B*T_out][2].
 * tdeed_sgp_gemm_gelu_chsum: out = GELU(A . W^T + b) (A bf16 [B*T][K], out in dtype_o); chs_out [NJ][B][N][2] per-channel
 *   (sum, sum of squares) of the stored rows of each row tile. */
int tdeed_sgp_gemm_ksteps(int K);
int tdeed_sgp_gemm_row_tiles(int T, int MT);
int tdeed_sgp_gemm_col_tiles(int N, int NT);
int tdeed_sgp_gemm_form(int mode, int B, int T, int N, int K);
int tdeed_sgp_gemm_gn_gelu(const void* y, int B, int T, int K, const float* chsum, int chs_parts, const float* gn_w,
                           const float* gn_b, int G, float eps, const void* Wp, const float* bias, int N, void* H, int form,
                           int dtype_a, void* stream);
int tdeed_sgp_gemm_residual(const void* H, int B, int T, int K, const void* Wp, const float* bias, int N, const void* resid,
                            void* out, float* rowstat_part, void* pooled, float* rowstat_pool_part, int T_out, int form,
                            int dtype_o, void* stream);
int tdeed_sgp_gemm_gelu_chsum(const void* A, int B, int T, int K, const void* Wp, const float* bias, int N, void* out,
                              float* chs_out, void* out16 /* optional bf16 copy of out */, int form, int dtype_o,
                              void* stream);

/* ---- baseline JPEG decode of a video's frames on the device (csrc/jpeg.hip, csrc/jpeg_core.h; tables and packing:
 * tdeed_amd/jpegdev.py).  sampling: 0 greyscale, 1 4:4:4, 2 4:2:2, 3 4:2:0.  A frame's coefficients are
 * tdeed_jpeg_frame_coeffs int16 values: per component the blocks of the padded MCU grid, row-major, 64 values each in
 * natural order, un-dequantised.
 * tdeed_jpeg_entropy: one lane per row of the segment table (int32 [n_segments][6]: frame, first MCU, MCU count, byte offset
 *   into stream, byte length, table set); waves int32 [n_waves][2] = (first row, count <= 64), the rows of a wave consecutive
 *   and of one table set; table_sets [n_sets][4240] bytes (JcTableSet).  Frames frame_lo .. frame_lo + n_frames - 1 decode into
 *   coeff (zero-filled by the caller on the same stream); rows of other frames get status 7.  status int32 [n_segments]:
 *   0, or 1 data exhausted, 2 marker inside the segment, 3 no code within 16 bits, 4 DC category > 11, 5 AC size > 10,
 *   6 run past 63, 7 row outside its buffers.  A lane never reads outside its segment nor stores outside its frame.
 * tdeed_jpeg_pixels: coeff of the same frame range -> out uint8 [all frames][3][H][W] rows frame_lo ..; dequantisation, integer
 *   IDCT, triangle up-sampling and YCbCr -> RGB, bit-identical to libjpeg-turbo's defaults.  frame_table_set int32 per
 *   frame of the whole video; a frame with a negative entry is left untouched (the caller decodes it on the host).
 * tdeed_jpeg_pixels_rows: the same kernel body with a row table: pack frame f (frame_lo <= f < frame_lo + n_frames) goes to
 *   out + dst_row[f] * 3*H*W, out uint8 [out_rows][3][H][W] (the rows i*T + t of a (B,T,3,H,W) clip-batch slot); a frame
 *   with dst_row[f] < 0, dst_row[f] >= out_rows or a negative table set stores nothing.  dst_row int32, one entry per
 *   frame of the whole pack, on the device.
 * tdeed_jpeg_pixels_window: tdeed_jpeg_pixels_rows over the window [top, top + wh) x [left, left + ww) of the frames: out uint8
 *   [out_rows][3][wh][ww].  Only the bands that hold window rows are launched and only the blocks under the window (and
 *   under the chroma samples its up-sampling taps touch) are transformed: coefficients of other blocks are never read.  The
 *   full window gives the bits of tdeed_jpeg_pixels_rows; an empty window or one that leaves the frame is an error.
 * tdeed_jpeg_window_blocks: those block ranges as ten ints (band_lo, band_n, luma block columns lo / n, luma block rows
 *   lo / hi, chroma block columns lo / n, MCU rows lo / hi with the 4:2:0 halo); 0, or -1 for a bad geometry or window.
 * tdeed_jpeg_pixels_lds_bytes: the dynamic LDS bytes per workgroup that tdeed_jpeg_pixels / tdeed_jpeg_pixels_rows (windowed
 *   0) or tdeed_jpeg_pixels_window (windowed 1) request for this geometry; -1 for a bad geometry or window. */
long tdeed_jpeg_frame_coeffs(int W, int H, int sampling);
int tdeed_jpeg_entropy(const uint8_t* stream, long stream_bytes, const int* segments, int n_segments, const int* waves,
                       int n_waves, const uint8_t* table_sets, int n_sets, int W, int H, int sampling, int frame_lo,
                       int n_frames, int16_t* coeff, int* status, void* hip_stream);
int tdeed_jpeg_pixels(const int16_t* coeff, const int* frame_table_set, const uint8_t* table_sets, int n_sets, uint8_t* out,
                      int frame_lo, int n_frames, int H, int W, int sampling, void* hip_stream);
int tdeed_jpeg_pixels_rows(const int16_t* coeff, const int* frame_table_set, const uint8_t* table_sets, int n_sets,
                           uint8_t* out, long out_rows, const int* dst_row, int frame_lo, int n_frames, int H, int W,
                           int sampling, void* hip_stream);
int tdeed_jpeg_pixels_window(const int16_t* coeff, const int* frame_table_set, const uint8_t* table_sets, int n_sets,
                             uint8_t* out, long out_rows, const int* dst_row, int frame_lo, int n_frames, int H, int W,
                             int sampling, int top, int left, int wh, int ww, void* hip_stream);
int tdeed_jpeg_window_blocks(int W, int H, int sampling, int top, int left, int wh, int ww, int* ranges);
long tdeed_jpeg_pixels_lds_bytes(int W, int H, int sampling, int windowed, int top, int left, int wh, int ww);

/* ---- entropy streams that stay on the device (trainclips.ResidentJpegClips).  A piece is a run of MCUs of one segment
 * that decodes on its own from a recorded decoder state; the piece table has 72-byte rows (JcPiece, csrc/jpeg_core.h:
 * int64 position of the next unread byte in the stream; int32 segment, first MCU, MCU count, table set, bytes left in the
 * segment, spare; the state: uint64 bits, int32 byte offset in the segment, valid bits n, pad, marker, three DC predictors,
 * spare).  MCU m of a segment starts a piece when m is its first MCU or m % split_mcus == 0.
 * tdeed_jpeg_entropy_index: one lane per row of `segments`, the rows of one shard whose byte offsets count from
 *   stream + base (stream_bytes: the whole resident stream, may exceed 2^31).  Stores no coefficients; writes the piece
 *   rows of row i at pieces[piece_off[i] ..] (piece_off int32 [n_segments + 1], below n_pieces; `segment` = seg_base + i)
 *   and status[i] as tdeed_jpeg_entropy does.
 * tdeed_jpeg_entropy_items: one lane per item; items int32 [n_items][2] = (piece row, coefficient slot), waves int32
 *   [n_waves][2] = (first item, count <= 64), the items of a wave of one table set.  Slots slot_lo .. slot_lo + n_slots - 1
 *   decode into coeff (zero-filled by the caller).  An item or row that points outside any buffer counts as status 7 and
 *   touches nothing; *err (uint32, on the device) gets bit `status` set for every non-zero status met.
 * tdeed_jpeg_entropy_items_reloc: the same decode where a piece's bytes are a staged copy.  reloc holds n_reloc 24-byte
 *   rows (JcReloc: int64 delta, lo, hi), indexed by the item's slot: the piece's bytes start at stream + pos - delta and
 *   must lie wholly in [lo, hi) of the stream, lo >= 0, hi <= stream_bytes; a piece that does not, or a slot >= n_reloc,
 *   counts as status 7 and touches nothing.  delta = 0 with the window (0, stream_bytes) is tdeed_jpeg_entropy_items.
 * tdeed_jpeg_slot_fill: rows of out uint8 [n_rows][frame_bytes] that no decode fills: fill[row] = -2 leaves the row, -1
 *   zeroes it, r >= 0 copies row r of side uint8 [side_rows][frame_bytes] (r >= side_rows stores nothing). */
int tdeed_jpeg_entropy_index(const uint8_t* stream, long stream_bytes, long base, const int* segments, int n_segments,
                             const int* waves, int n_waves, const uint8_t* table_sets, int n_sets, int W, int H, int sampling,
                             int split_mcus, const int* piece_off, int seg_base, void* pieces, int n_pieces, int* status,
                             void* hip_stream);
int tdeed_jpeg_entropy_items(const uint8_t* stream, long stream_bytes, const void* pieces, int n_pieces, const int* items,
                             int n_items, const int* waves, int n_waves, const uint8_t* table_sets, int n_sets, int W, int H,
                             int sampling, int slot_lo, int n_slots, int16_t* coeff, unsigned* err, void* hip_stream);
int tdeed_jpeg_entropy_items_reloc(const uint8_t* stream, long stream_bytes, const void* pieces, int n_pieces,
                                   const int* items, int n_items, const int* waves, int n_waves, const uint8_t* table_sets,
                                   int n_sets, int W, int H, int sampling, int slot_lo, int n_slots, const void* reloc,
                                   int n_reloc, int16_t* coeff, unsigned* err, void* hip_stream);
int tdeed_jpeg_slot_fill(const uint8_t* side, long side_rows, long frame_bytes, const int* fill, int n_rows, uint8_t* out,
                         void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
