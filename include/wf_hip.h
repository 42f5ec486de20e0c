/*
 * libwf_hip.so -- C-ABI of the MI355X-native WorldForge guided-denoising hot path.
 *
 * The reference (Westlake-AGI-Lab/WorldForge) is pure Python and has no FFI of its own; the drop-in
 * boundary is therefore the set of tensor operations its sampler executes eagerly through PyTorch
 * (SURVEY.md section 8b).  Every entry point below names the reference statement(s) it replaces
 * (paths relative to /root/reference/wan_for_worldforge):
 *   PIPE  = utils/pipeline_wan_i2v_clean.py
 *   SCHED = utils/scheduling_unipc_multistep_clean.py
 *   DIT   = wan/modules/model.py (+ attention.py)  -- in-tree statement of diffusers' WanTransformer3DModel
 *   VAE   = wan/modules/vae.py                     -- in-tree statement of diffusers' AutoencoderKLWan
 *
 * Conventions
 *   - plain pointers and sizes only; all tensor pointers are DEVICE pointers owned by the caller
 *     (the Python host allocates them with the PyTorch-ROCm caching allocator);
 *   - contiguous row-major tensors unless a stride argument is given;
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous on that stream;
 *   - return value: 0 = WF_OK, negative = WF_E*; text via wf_last_error(); nothing ever falls back
 *     silently to another implementation (contrast SCHED:1284-1295, 1419-1421);
 *   - no hidden host synchronisation and no allocation inside any call; reductions use a fixed tree
 *     order (no floating-point atomics) so repeated runs are bit-identical;
 *   - `rb*` flags: "this intermediate is a bfloat16 torch tensor in the reference", i.e. its value is
 *     rounded to bf16 (round-to-nearest-even) exactly where eager PyTorch would round it.
 */
#ifndef WF_HIP_H_
#define WF_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WF_OK 0
#define WF_EINVAL (-1)   /* bad argument (shape / dtype / alignment) */
#define WF_EHIP (-2)     /* a HIP runtime call or kernel launch failed */
#define WF_ENOTSUP (-3)  /* configuration not built */

#define WF_F32 0
#define WF_BF16 1

/* ---- library ------------------------------------------------------------------------------- */
int wf_version(void);
const char* wf_last_error(void);
/* Number of compute units / name of device `dev` (host query, used by bench/roofline). */
int wf_device_info(int dev, int* n_cu, int* clock_khz, char* name, int name_len);

/* ---- scheduler / injection element-wise set (HBM-bound; latent tensors are [B,16,T,h,w]) -- */

/* PIPE:611  noise_pred = cond + g * (cond - uncond).  Element dtype `dt` for all three. */
int wf_cfg_combine(const void* cond, const void* uncond, void* out, int dt, float g, size_t n, void* stream);

/* SCHED:952-958  x0 = sample - sigma * v.   dt_v / dt_s: dtypes of v and sample; out has the torch-promoted dtype
 * (bf16 only if both are bf16). */
int wf_x0_from_v(const void* sample, int dt_s, const void* v, int dt_v, void* out, float sigma, size_t n,
                 void* stream);

/* SCHED:1083-1098 (predict_x0, bh2)  x_t = c1*x - c2*m0 - c3 * 0.5 * (m1 - m0)/rk   (order 2; m1 == NULL -> order 1)
 *   c1 = sigma_t/sigma_s0, c2 = alpha_t*expm1(-h), c3 = alpha_t*B_h, rk = (lambda_s1-lambda_s0)/h computed by the host in
 *   fp32 exactly as SCHED:1016-1069 does.  out has x's dtype (SCHED:1098). */
int wf_unipc_update(const void* x, int dt_x, const void* m0, int dt_m0, const void* m1, int dt_m1, void* out, float c1,
                    float c2, float c3, float rk, size_t n, void* stream);

/* SCHED:1584  noisy = (1 - sigma) * x0 + sigma * noise.  `one_minus_sigma` and `sigma` are supplied by the host already
 * rounded to x0's dtype (SCHED:1552).  out dtype = promote(x0, noise). */
int wf_add_noise(const void* x0, int dt_x0, const void* noise, int dt_n, void* out, float one_minus_sigma, float sigma,
                 size_t n, void* stream);

/* SCHED:1281 (dir 0: z / istd[c] + mean[c] -> f32 out)  and  SCHED:1385, PIPE:351 (dir 1: (z - mean[c]) * istd[c]).
 * z is [B,C,inner]; mean/istd are HOST arrays of C floats (<= 64). in dtype dt_in, out dtype dt_out. */
int wf_latent_affine(const void* z, int dt_in, void* out, int dt_out, const float* mean, const float* istd, int dir, int B,
                     int C, size_t inner, void* stream);

/* SCHED:1375-1380  fused = (2*ref - 1) * mask + dec * (1 - mask);  ref, dec, out: [B,3,inner] f32, mask: [B,1,inner] f32. */
int wf_blend_pixels(const float* ref, const float* mask, const float* dec, float* out, int B, int C, size_t inner,
                    void* stream);

/* Which pixel columns of the decoded video the blend above can see: wherever mask == 1 (exactly) the result is (2 ref - 1) + dec * 0, i.e.
 * independent of any finite dec.  mask [n_rows, W] f32 (all frames and rows of a job's mask) -> out2 (DEVICE, 2 ints) = {first column with a
 * pixel != 1, last such column + 1}; {W, 0} when every pixel is 1.  What lets the VAE decode only the columns an IRR injection consumes
 * (worldforge_amd/vae.py decode(columns=...)). */
int wf_mask_column_range(const float* mask, size_t n_rows, int W, int* out2, void* stream);

/* PIPE:744 (diffusers VideoProcessor.postprocess_video)  out = clamp(x/2 + 0.5, 0, 1), [C,F,H,W] -> [F,H,W,C]. */
int wf_postprocess_video(const float* x, float* out, int C, int F, int H, int W, void* stream);
/* The two pixel-space statements above as eager PyTorch evaluates them behind a BF16 VAE module -- the dtype the LongCat entry loads its
 * VAE in (longcat_for_worldforge/run_longcat_worldforge_single.py:205): dec / out bf16, the fp32 ref and mask rounded to bf16 first
 * (longcat_video/modules/scheduling_flow_match_euler_discrete.py:1152-1153) and every statement of :1156-1164 rounded to bf16;
 * the post-processing of a bf16 video (pipeline_longcat_video.py:1002) likewise, returned as f32. */
int wf_blend_pixels_bf16(const float* ref, const float* mask, const void* dec, void* out, int B, int C, size_t inner, void* stream);
int wf_postprocess_video_bf16(const void* x, float* out, int C, int F, int H, int W, void* stream);

/* dtype conversion / bf16 rounding of latent-shaped tensors (PIPE:590 .to(bf16), PIPE:708). */
int wf_cast(const void* in, int dt_in, void* out, int dt_out, size_t n, void* stream);

/* SCHED:1410-1412  enc[:, c] = pred[:, c] for the listed channels (host array, n_idx <= C). Tensors [B,C,inner]. */
int wf_channel_swap(void* enc, int dt_enc, const void* pred, int dt_pred, const int* idx, int n_idx, int B, int C,
                    size_t inner, void* stream);

/* ---- resize (SCHED:1316-1324 bilinear align_corners=False for the reference video; SCHED:1355-1362 nearest for the mask).
 * The temporal branches SCHED:1326-1334 / 1364-1371 call F.interpolate with a 3-element size on a 4-D tensor and raise
 * ValueError in the reference, so a frame-count mismatch is an error here too (raised by the Python host). */
int wf_resize_bilinear2d(const float* in, float* out, int N, int Hi, int Wi, int Ho, int Wo, void* stream);
int wf_resize_nearest2d(const float* in, float* out, int N, int Hi, int Wi, int Ho, int Wo, void* stream);

/* ---- front end: soften_mask (infer_worldforge.py:105-150) -------------------------------------------------------------- */
/* mask [F,H,W] f32 (any non-zero = inside) -> out [F,H,W]: inside pixels within transition_distance of the zero region get
 * ramp(d / transition_distance), d = exact Euclidean distance to the nearest zero pixel of the frame (float64 like scipy's EDT);
 * decay_type 0 linear, 1 exponential (1 - e^-3t), 2 sine, 3 cosine.  mask and out may not alias. */
int wf_soften_mask(const float* mask, float* out, int F, int H, int W, int transition_distance, int decay_type, void* stream);

/* ---- DSG (PIPE:664-681) ---------------------------------------------------------------------- */
/* Workspace floats needed by wf_dsg (partials + 8 result floats). */
size_t wf_dsg_workspace_floats(void);
/* One call = reduce (dot, |g|^2, |w|^2 in a fixed tree) -> coefficients on device -> apply:
 *   better = g + omega*sin(theta) * (g - (|g|/(|w|+1e-8))*cos(theta) * w).   g = "good" (post-injection), w = "worse".
 * ws: wf_dsg_workspace_floats() floats; ws[0..7] afterwards = {dot, ng2, nw2, cos, sin, ratio, 0, 0} for inspection. */
int wf_dsg(const void* g, const void* w, void* out, int dt, float omega, size_t n, float* ws, void* stream);
/* CFG-zero (LongCat pipeline_longcat_video.py:374-383 optimized_scale + :875-888): st = <cond,uncond> / (|uncond|^2 + 1e-8) over the
 * whole sample; out = uncond*st + guidance*(cond - uncond*st), negated when negate != 0 (the sign flip of :888).  fp32;
 * ws: wf_dsg_workspace_floats() floats, ws[0..3] afterwards = {dot, |cond|^2, |uncond|^2, st}. */
int wf_cfg_zero(const float* cond, const float* uncond, float* out, float guidance, int negate, size_t n, float* ws, void* stream);

/* ---- FLF metric (SCHED:497-607) ------------------------------------------------------------------ */
/* Temporal-difference motion (SCHED:391-392, 478-479): out[c,t,:] = x[c,t+1,:] - x[c,t,:];  x [C,T,hw] -> out [C,T-1,hw] f32. */
int wf_temporal_diff(const void* x, int dt, float* out, int C, int T, size_t hw, void* stream);
size_t wf_flow_metrics_workspace_floats(int n_channels);
/* For each of n_channels: ref flow [Tm, Cr, hw], chan flow [Tm, Cc, hw] (Cr, Cc in {1,2}; 1 is replicated to 2 as SCHED:531-539),
 * similarity = 1 - (.45*clamp(mEPE/10) + .45*clamp(Fl/.5) + .1*clamp(mAE/30))  -> sim[n_channels] (device floats). */
int wf_flow_metrics(const float* ref_flow, const float* chan_flow, float* sim, int n_channels, int Tm, int Cr, int Cc,
                    size_t hw, float* ws, void* stream);
/* The same with the metric variant selectable: 0 = the Wan scheduler's (above); 1 = the LongCat scheduler's
 * (longcat_video/modules/scheduling_flow_match_euler_discrete.py:172-243): outlier = (epe > 3) OR (epe > 5 % |ref|),
 * similarity = 1 - (.4*clamp(mEPE/10) + .4*clamp(Fl/.5) + .2*clamp(mAE/30)). */
int wf_flow_metrics_variant(const float* ref_flow, const float* chan_flow, float* sim, int n_channels, int Tm, int Cr, int Cc,
                            size_t hw, int variant, float* ws, void* stream);

/* ---- FLF optical flow (SCHED:156-248) ----------------------------------------------------------------------------------
 * What `cv2.calcOpticalFlowFarneback(g1, g2, None, 0.5, 3, 15, 3, 5, 1.2, 0)` (SCHED:220-224) computes for every consecutive frame
 * pair of every channel of a latent tensor, including the reference's preparation of its input: normalisation by the tensor's
 * global min / range (SCHED:376-388, 462-474), x255, truncation to uint8 (SCHED:175), RGB2GRAY of three equal channels.
 * x [C,T,h,w] (f32 / bf16) -> flow [C, T-1, 2, h, w] f32 (x then y displacement, the layout of SCHED:240-244).
 * OpenCV is a third-party dependency absent from the reference tree: parity with a real cv2 is UNPINNED.
 * quant_mode selects the reference's uint8 preparation: 0 = Wan (above); 1 = LongCat-Video (LSCHED:105-121, 290-297): min / range per
 * CHANNEL, normalised in the tensor's own dtype (bf16 arithmetic on a bf16 tensor), then uint8(clip((n + 1) * 127.5, 0, 255)); C <= 64. */
size_t wf_farneback_workspace_bytes(int C, int T, int h, int w);
int wf_farneback_flows(const void* x, int dt, float* flow, int C, int T, int h, int w, int quant_mode, void* ws, void* stream);


/* ---- DiT (wan/modules/model.py; the in-tree statement of diffusers' WanTransformer3DModel) --------------------------- */
#define WF_EPI_BF16 0       /* out bf16 = acc + bias */
#define WF_EPI_BF16_GELU 1  /* out bf16 = gelu_tanh(acc + bias)            (model.py:272) */
#define WF_EPI_F32 2        /* out f32  = acc + bias */
#define WF_EPI_RESID 3      /* out f32 += (acc + bias) * gate[n] (gate NULL -> 1)   (model.py:306, 310, 313) */
#define WF_EPI_F32_ACC 4    /* out f32 += acc + bias */
/* nn.Linear on MFMA (model.py:123-126, 271-273, 332, 456-464; vae.py 1x1 convs): out[M,N] = epi(X[M,K] . W[N,K]^T + bias).
 * X, W bf16 (row strides ldx, ldw); bias/gate f32; K % 8 == 0, N % 4 == 0, 16-byte aligned pointers. */
int wf_gemm_bf16(const void* X, const void* W, const float* bias, void* out, const float* gate, int M, int N, int K, int ldx,
                 int ldw, int ldo, int epilogue, void* stream);
/* `batch` independent small products in one launch: out_b = X_b . W_b^T with problem b at X + b*bsx, W + b*bsw, out + b*bso elements;
 * epilogue WF_EPI_BF16 or WF_EPI_F32, no bias.  The per-head block-score products of the block-sparse gating
 * (bsa_interface.py:181-185: one [n_q, 128] x [n_k, 128]^T per head) and the per-frame score / PV products of the VAE mid-block. */
int wf_gemm_bf16_batched(const void* X, const void* W, void* out, int batch, int M, int N, int K, int ldx, int ldw, int ldo,
                         int64_t bsx, int64_t bsw, int64_t bso, int epilogue, void* stream);
/* wf_gemm_bf16 on fp16 operands (X, W fp16; fp32 accumulation; epilogue WF_EPI_BF16 writes fp16, WF_EPI_F32, WF_EPI_F32_ACC): the
 * 1x1 convolutions and mid-block attention products of the VAE in its fp16 operand formats (see wf_split_f16x3).  acc_scale (round 5;
 * 1 = none): out = epilogue(acc * acc_scale + bias) -- 2^-k for a weight operand stored scaled by 2^k (see "fp16 operand formats"). */
int wf_gemm_f16(const void* X, const void* W, const float* bias, void* out, int M, int N, int K, int ldx, int ldw, int ldo, int epilogue,
                float acc_scale, void* stream);
/* wf_gemm_bf16_batched on fp16 operands (WF_EPI_BF16 writes fp16): the per-frame P . V products of the VAE mid-block attention
 * (vae.py:252-258) of all frames in one launch. */
int wf_gemm_f16_batched(const void* X, const void* W, void* out, int batch, int M, int N, int K, int ldx, int ldw, int ldo, int64_t bsx,
                        int64_t bsw, int64_t bso, int epilogue, void* stream);
/* Opt-in MX-fp8 linear layers (csrc/mxfp8.hip; OCP MX: e4m3fn elements, one E8M0 scale 2^e per 32 consecutive K elements of a row).
 * wf_mx_quant_e4m3: X bf16 [M, K] (row stride ldx % 8 == 0, 16-byte aligned) -> Q e4m3 [M, K] (8-byte aligned) + S E8M0 [M, K/32]; K % 32 == 0.
 * e = the smallest integer with amax / 2^e <= 448, clamped to [-127, 127]; elements x / 2^e rounded to nearest even; an all-zero block
 * gets scale byte 0; a block holding a NaN / Inf gets scale 0xff (E8M0 NaN) and NaN elements (0x7f). */
int wf_mx_quant_e4m3(const void* X, void* Q, void* S, int M, int K, int ldx, void* stream);
/* out[M,N] = epi(dequant(Xq, Xs) . dequant(Wq, Ws)^T + bias), fp32 accumulation; epilogue WF_EPI_BF16 / _BF16_GELU / _F32 / _RESID as
 * wf_gemm_bf16.  Xq / Wq e4m3 with row strides ldx / ldw (bytes, % 16 == 0, 16-byte aligned), scales [rows, K/32] (4-byte aligned);
 * K % 128 == 0, N % 4 == 0; anything else returns WF_EINVAL. */
int wf_gemm_mxfp8(const void* Xq, const void* Xs, const void* Wq, const void* Ws, const float* bias, void* out, const float* gate, int M, int N,
                  int K, int ldx, int ldw, int ldo, int epilogue, void* stream);
/* Switchable LoRA adapters on resident weights (csrc/lora.hip; longcat_video_dit.py:194-270, lora_utils.py:15-78 as a weight switch):
 *   out[n,k] = bf16_rne(base[n,k] + sum_j scale_j * sum_r U_j[n,r] * D_j[(n / (N / nsep_j)) * rank_j + r, k]),  j < n_adapters (1..4)
 * for one bf16 matrix [N, K] or a contiguous row slice of one (contiguous rows, K % 8 == 0).  U_j bf16 [N, rank_j], D_j bf16
 * [nsep_j * rank_j, K] (row block b of a fused qkv / kv weight uses rank slice b: LoRAUPParallel), rank_j a multiple of 8 in 8..256,
 * N % nsep_j == 0, all pointers 16-byte aligned.  bf16 MFMA products, fp32 accumulation / scaling / base add, ONE rounding.  base is
 * only read; out may be base.  The slots j >= n_adapters are ignored.  Anything else returns WF_EINVAL before any device work. */
int wf_lora_fold(const void* base, void* out, int N, int K, int n_adapters, const void* U0, const void* D0, int rank0, int nsep0,
                 float scale0, const void* U1, const void* D1, int rank1, int nsep1, float scale1, const void* U2, const void* D2,
                 int rank2, int nsep2, float scale2, const void* U3, const void* D3, int rank3, int nsep3, float scale3, void* stream);

/* flash_attention (attention.py:24-130) as used by model.py:149-154 (self) and :220-222 (cross): fused
 * softmax(Q K^T * softmax_scale) V, no mask, head_dim 128.  Q [H][Lq][128], K [H][Lkp][128],
 * Vt [H][Lkp/64][128][64] (wf_v_transpose), O [Lq][ldo] bf16 with head h at columns h*128 (ldo % 8 == 0, O 16-byte aligned: 16-byte stores).
 * Padding contract (all attention entry points; pinned by tests/test_gpu_attn_fp64.py): the kernel masks the scores of the keys >= kv_len
 * of the last 64-key tile to -inf itself, so K's rows and V^T's key columns kv_len .. ceil(kv_len/64)*64 - 1 may hold ANY FINITE values
 * (p = 0 times a finite v is 0; an inf or NaN there would leak as 0 * inf) -- the producers zero them (wf_rmsnorm_heads leaves rows
 * L..Lout of a zeroed buffer untouched, wf_v_transpose zero-fills), but no result depends on that.  Whole tiles behind
 * ceil(kv_len/64) (Lkp larger than needed) are never read.
 * accumulate != 0: O += result.
 * seg_len: Lkp for one contiguous K/V; with sequence parallelism K/V are the all-gathered per-rank shards [P][H][seg_len][128]
 * (seg_len % 64 == 0, Lkp = P*seg_len) and key index = seg*seg_len + row.
 * softmax_scale = 0: Q already carries softmax_scale * log2(e) (wf_rmsnorm_heads out_scale) -- the score accumulators then start
 * from -m instead of 0 and hold s - m directly, which takes one VALU instruction per score out of the softmax.
 * seg_stride_bytes (round 5): 0 = the dense [P][H][seg_len][128] form above; otherwise the bytes from one segment's head 0 to the next
 * segment's head 0, the SAME for K and Vt -- each source rank's K shard, V^T shard and norm-bound vector then travel as ONE packed slot
 * [K | V^T | bounds] of an exchange buffer (one collective and one event per source or per chunk; worldforge_amd/parallel.py KVExchange),
 * K and Vt point into slot 0.  kmax_stride: floats between two kmax2 vectors (0 = H, contiguous). */
int wf_attn_fwd(const void* Q, const void* K, const void* Vt, void* O, int H, int Lq, int Lkp, int kv_len, int seg_len,
                size_t seg_stride_bytes, int ldo, float softmax_scale, int accumulate, const float* kmax2, int kmax_n, int kmax_stride,
                const float* qmax2, int qmax_n, void* stream);
/* Per-head max over the rows of |x|^2: X bf16 [H][Lp][128] (rows >= L ignored) -> out f32 [H], which the caller zeroes first.
 * Computed for K and for the pre-scaled Q and handed to wf_attn_fwd (softmax_scale = 0 only) as kmax2 / qmax2 -- kmax_n / qmax_n such
 * vectors each, one per shard when the tensor is all-gathered -- it lets the kernel prove by Cauchy-Schwarz that no score of the head
 * can overflow: B = max|q| max|k| bounds |s|, a row's reference max is >= -B, so s - m <= 2B; with 2B <= 100 (exp2 domain) the
 * workgroup runs WITHOUT the running-max tracking of the online softmax (exact: the same m is used for P and the row sum).  The tracked
 * path remains the fallback (larger norms, NaNs) and the only path when either pointer is NULL. */
int wf_head_max_norm2(const void* X, int H, int L, int Lp, float* out, void* stream);
/* The same with the KV sweep split nsplit ways (each split leaves un-normalised partials in the workspace, a merge kernel combines
 * them exactly): fills the chip when Lq is short, e.g. one rank's token shard of the sequence-parallel DiT (Lq = 4096 at 8 ranks:
 * 640 workgroups on 256 CUs).  workspace: wf_attn_split_workspace_bytes(H, Lq, nsplit) bytes, 16-byte aligned. */
size_t wf_attn_split_workspace_bytes(int H, int Lq, int nsplit);
/* WanI2VCrossAttention (model.py:202-229) in ONE launch: O = softmax(Q K1^T s) V1 + softmax(Q K2^T s) V2 for the image context (K1, 257
 * keys) and the text context (K2, 512 keys), where the reference runs two flash_attention calls and adds (model.py:220-227).  K [H][Lk1p +
 * Lk2p][128] holds context 1 (kv_len1 valid rows of Lk1p, padded to whole 64-key tiles with finite values: see the padding contract at wf_attn_fwd) followed by context 2; Vt [H][(Lk1p + Lk2p) /
 * 64][128][64] likewise (wf_v_transpose_seg).  Q is read once and O written once; context 1's normalised result is rounded to bf16 and kept
 * in registers across the seam, so the result is bit-identical to wf_attn_fwd(context 1) followed by wf_attn_fwd(context 2, accumulate). */
int wf_attn_cross2_fwd(const void* Q, const void* K, const void* Vt, void* O, int H, int Lq, int Lk1p, int kv_len1, int Lk2p, int kv_len2,
                       int ldo, float softmax_scale, void* stream);
/* Test hook: counters2 = device uint32[2] (or NULL = off, the default).  While set, every workgroup of a pre-scaled-Q launch
 * (wf_attn_fwd / wf_attn_fwd_split with softmax_scale = 0) adds 1 to counters2[0] if it ran the max-tracking body and to counters2[1]
 * if it ran the un-tracked one -- lets a parity test assert WHICH body it compared with the oracle.  Process-global, not thread-safe. */
int wf_attn_debug_body_counter(void* counters2);
int wf_attn_fwd_split(const void* Q, const void* K, const void* Vt, void* O, int H, int Lq, int Lkp, int kv_len, int seg_len,
                      size_t seg_stride_bytes, int ldo, float softmax_scale, int accumulate, int nsplit, void* workspace, const float* kmax2,
                      int kmax_n, int kmax_stride, const float* qmax2, int qmax_n, void* stream);
/* The KV sweep in PARTS (round 4; sequence-parallel layers WITHOUT a second CFG branch to hide the K / V^T exchange under -- LongCat-Video,
 * distilled schedules, guidance_scale <= 1; reference idea: wan/distributed/xdit_context_parallel.py:160-176, pipeline_longcat_video.py:
 * 857-866).  The key segments arrive one source rank after the other; a part launch walks only the 64-key tiles [t_begin, t_end) that are
 * there already -- the rank's own shard needs no wait at all -- and leaves un-normalised partials (O f32, reference max, row sum) in the
 * slots `part` ... `part + inner_splits - 1` of an `nparts`-slot workspace of wf_attn_split_workspace_bytes(H, Lq, nparts) bytes
 * (inner_splits >= 1 halves / thirds the window over blockIdx.y so that a short query shard fills whole rounds of workgroups).  Pre-scaled Q only (the form of
 * wf_attn_fwd with softmax_scale = 0); Q / K / Vt / bounds as wf_attn_fwd.  wf_attn_merge combines the slots exactly (the flash combine
 * wf_attn_fwd_split uses) into O once every slot has been written; the result equals the one-launch sweep up to the re-association of the
 * fp32 partial sums.
 * Round 5: nparts up to 12; an optional SECOND window [t_begin2, t_end2) (t_end2 <= t_begin2: none) behind the first -- the keys on the far
 * side of a hole, i.e. of the rank's own segment(s), which an earlier part launch walked without waiting for the exchange: one launch then
 * covers "every peer" of an all-gathered buffer.  seg_stride_bytes / kmax_stride as wf_attn_fwd.
 * Round 6: the two windows are walked as ONE sequence by the same workgroups (the hole must be whole segments): `inner_splits` splits of
 * the joined sequence fill the slots part ... (n tiles in k splits: ceil(n / ceil(n / k)) slots) -- one slot and one prologue / epilogue
 * per peer chunk where round 5 spent two.  O_merge != NULL (the LAST launch of a sweep: part = nparts - 1, one split): the launch folds
 * the slots 0 .. part - 1 into its own result in its epilogue and writes the normalised bf16 rows to O_merge [Lq][ldo] -- no partial, no
 * separate wf_attn_merge pass. */
int wf_attn_fwd_part(const void* Q, const void* K, const void* Vt, int H, int Lq, int Lkp, int kv_len, int seg_len, size_t seg_stride_bytes,
                     int t_begin, int t_end, int t_begin2, int t_end2, int inner_splits, int part, int nparts, void* workspace, void* O_merge,
                     int ldo, const float* kmax2, int kmax_n, int kmax_stride, const float* qmax2, int qmax_n, void* stream);
int wf_attn_merge(void* O, int H, int Lq, int ldo, int accumulate, int nparts, const void* workspace, void* stream);

/* WanLayerNorm (model.py:92-102; eps, no affine) fused with y = ln * (plus_one + mul[c]) + add[c]:
 *   AdaLN modulate (model.py:303, 311, 346): mul = scale e[1]/e[4], add = shift e[0]/e[3], plus_one = 1;
 *   affine LayerNorm (norm3 :262-264, img_emb :356-358): mul = weight, add = bias, plus_one = 0.
 * x f32 [L,C]; out bf16 or f32 [L,C]. */
int wf_ln_modulate(const float* x, const float* mul, const float* add, void* out, int out_dtype, int L, int C, float eps,
                   int plus_one, void* stream);

/* WanRMSNorm over all C channels (model.py:73-89, 142-143, 215-218) + optional 3-axis RoPE (model.py:43-70; cos/sin tables
 * [L][64] f32, NULL -> none), written head-major: in bf16 [L, ld] -> out bf16 [C/128][Lout][128] (rows L..Lout untouched).
 * out_scale (1 = none) multiplies the f32 result in front of the one bf16 rounding: the self-attention Q is produced as
 * q * head_dim^-1/2 * log2(e), and wf_attn_fwd is then called with softmax_scale = 0 ("Q is pre-scaled"). */
int wf_rmsnorm_heads(const void* in, int ld, const float* weight, const float* cos_tab, const float* sin_tab, void* out, int L,
                     int Lout, int C, float eps, float out_scale, void* stream);
/* The same, and in the same pass max_norm2[h] = max over the L rows of |out row of head h|^2 (of the values as stored, after the bf16
 * rounding) -- what wf_head_max_norm2 computes with a second pass over the tensor (rows holding NaN / inf report +inf likewise).
 * ws: wf_rmsnorm_heads_bound_ws_floats(L, C) floats.  C / 128 heads <= 64. */
size_t wf_rmsnorm_heads_bound_ws_floats(int L, int C);
int wf_rmsnorm_heads_bound(const void* in, int ld, const float* weight, const float* cos_tab, const float* sin_tab, void* out, int L, int Lout,
                           int C, float eps, float out_scale, float* ws, float* max_norm2, void* stream);

/* V [L, ld] bf16 (head h at columns h*128) -> Vt [H][Lp/64][128][64] bf16, keys >= L zero-filled (finite is all wf_attn_fwd needs). */
int wf_v_transpose(const void* V, int ld, void* Vt, int L, int Lp, int H, void* stream);
/* The same into a destination whose heads are head_stride_tiles 64-key tiles apart (Vt points at the segment's first tile of head 0): the
 * two contexts of wf_attn_cross2_fwd share one buffer. */
int wf_v_transpose_seg(const void* V, int ld, void* Vt, int L, int Lp, int H, int head_stride_tiles, void* stream);
/* APPEND at an arbitrary key offset (csrc/longcat_ops.hip; LongCat video continuation, attention.py:149-181: the condition frames' keys
 * [0, k0) of K / V^T stay resident across the denoising steps and each step's noise keys follow at k0 = condition tokens, in general
 * not a multiple of 64): V [L, ld] bf16 (head h at columns h*128) -> keys [k0, k0 + L) of Vt [H][Lp/64][128][64].  Keys < k0 keep their
 * bits, those sharing the first touched tile included (never read, never written: per-key stores where k0 cuts an 8-key chunk); keys
 * k0 + L .. end of the last touched tile are zero-filled; later tiles are not touched.  k0 = 0: the bits of wf_v_transpose in every tile
 * below ceil(L / 64).  WF_EINVAL before any device work unless k0 >= 0, L > 0, k0 + L <= Lp, Lp % 64 == 0, ld % 8 == 0, ld >= H * 128,
 * non-null 16-byte aligned pointers. */
int wf_v_transpose_at(const void* V, int ld, void* Vt, int k0, int L, int Lp, int H, void* stream);

/* model.py:534-537 patch embedding as a GEMM: x bf16 [Cin,T,Hh,Ww] -> tokens bf16 [T*(Hh/2)*(Ww/2), Cin*4] (k = c*4+ph*2+pw). */
int wf_patchify(const void* x, void* tokens, int Cin, int T, int Hh, int Ww, void* stream);
/* model.py:584-607: y f32 [L, 4*Cout] (k = (ph*2+pw)*Cout + c) -> out f32 [Cout,T,Hh,Ww]. */
int wf_unpatchify(const float* y, float* out, int Cout, int T, int Hh, int Ww, void* stream);

/* out = f(a (+ b)); mode 0 SiLU (model.py:463-464), 1 GELU-erf (model.py:357), 2 identity (e = modulation + e0, model.py:298). */
int wf_act(const void* a, int dt_a, const void* b, int dt_b, void* out, int dt_out, int mode, size_t n, void* stream);

/* ---- LongCat-Video DiT companions (longcat_for_worldforge/longcat_video/modules; LCD = longcat_video_dit.py, LCA = attention.py,
 *      LCB = blocks.py, LCR = rope_3d.py).  The LongCat residual stream is bf16 and its AdaLN parameters are per latent frame. ---- */
/* LayerNorm_FP32 (LCB:55-68) fused with y = ln * (plus_one + mul[g][c]) + add[g][c], g = (row0 + row) / rows_per_group (0: one group;
 * row0 = global index of the first row when x is one rank's token shard; group_index (int32 per GLOBAL row, may be NULL) replaces the
 * division when the rows are not in frame order -- the 3D-block token order of the refine pass):
 *   modulate_fp32 with per-frame shift / scale (LCB:133-141 as called at LCD:91, 114 and LCB:165): mul = scale, add = shift,
 *   mod_ld = floats between consecutive frames, rows_per_group = tokens per frame, plus_one = 1;
 *   affine pre_crs_attn_norm (LCD:111): mul = weight, add = bias, rows_per_group = 0, plus_one = 0.   x, out bf16 [L, C]. */
int wf_lc_ln_modulate(const void* x, const float* mul, const float* add, int64_t mod_ld, int rows_per_group, int64_t row0,
                      const int* group_index, int plus_one, void* out, int L, int C, float eps, void* stream);
/* x = bf16(x + gate[(row0 + row) / rows_per_group][c] * y) (LCD:102-104, 117-120); gate NULL: x = bf16(x + y) (LCD:111).
 * x bf16 [L, C] in place; y bf16 [L, ldy]; gate f32 rows gate_ld floats apart. */
int wf_lc_gate_residual(void* x, const void* y, int64_t ldy, const float* gate, int64_t gate_ld, int rows_per_group, int64_t row0,
                        const int* group_index, int L, int C, void* stream);
/* RMSNorm_FP32 over each head's 128 channels (LCB:40-52 as used at LCA:111 and LCA:231) + optional interleaved 3D RoPE
 * (LCR:32-36, 101-120; cos/sin tables [L][64] f32 per rotation pair, NULL -> none), written head-major for wf_attn_fwd:
 * in bf16 [L, ld] (head h at columns h*128) -> out bf16 [H][Lout][128] (rows L..Lout untouched); weight f32 [128].  out_scale multiplies the
 * result in front of its one bf16 rounding (1 = none; softmax_scale * log2(e) for the queries of wf_attn_fwd's softmax_scale = 0 form). */
int wf_lc_norm_heads(const void* in, int64_t ld, const float* weight, const float* cos_tab, const float* sin_tab, void* out, int L,
                     int Lout, int H, float eps, float out_scale, void* stream);
/* FeedForwardSwiGLU gate (LCB:36-37): in bf16 [L, ld] with w1 x in columns [0, Hd) and w3 x in [Hd, 2 Hd) ->
 * out bf16 [L, Hd] = silu(w1 x) * w3 x. */
int wf_lc_swiglu(const void* in, int64_t ld, void* out, int L, int Hd, void* stream);

/* LongCat refine pass input (pipeline_longcat_video.py:1407-1413): stage-1 frames uint8 [F][H0][W0][3] -> bilinear (align_corners) to
 * (H, W) -> / 255 -> linear along the frame axis (the trilinear of :1412 with H, W unchanged) to Fo frames -> * 2 - 1, every step
 * rounded to bf16 as the reference's bf16 tensors.  out f32 [3][Fo][H][W]. */
int wf_refine_upsample_u8(const void* frames_u8, float* out, int F, int H0, int W0, int Fo, int H, int W, void* stream);

/* ---- LongCat block-sparse attention of the 720p refine pass (longcat_video/block_sparse_attention/bsa_interface.py = BSA) --------- */
/* mean_pooling_compression (BSA:169-179): in bf16 [H][L][128] -> out bf16 [H][L/block][128], mean of each block of 64 / 128 tokens. */
int wf_lc_mean_pool_blocks(const void* in, void* out, int H, int L, int block, void* stream);
/* The same pooling (BSA:169-179) appended into a region of a wider destination: head h's L rows start at in + h * in_head_stride_rows
 * rows, their L / block means become blocks [b0, b0 + L / block) of out bf16 [H][out_head_stride_blocks][128]; no other block of out
 * is read or written.  Arithmetic and rounding of wf_lc_mean_pool_blocks (the same bits with b0 = 0 and dense strides).  WF_EINVAL
 * before any device work for: non-positive sizes, block not 64 / 128, L % block, in_head_stride_rows < L, b0 < 0 or b0 + L / block >
 * out_head_stride_blocks, null or not 16-byte aligned pointers. */
int wf_lc_mean_pool_blocks_at(const void* in, int64_t in_head_stride_rows, void* out, int out_head_stride_blocks, int b0, int H, int L,
                              int block, void* stream);
/* Block selection (BSA:211-224, `torch.topk(score, int((1 - sparsity) * n_k))`) fused with the list building of the sparse kernel:
 * scores bf16 [heads][n_q][ld] (n_k valid columns: the gating products of BSA:181-185) -> for every group of g = 256 / block consecutive
 * query blocks the ascending union of their n_sel best key blocks, entry = physical_block * 2^g + sum_i 2^i [selected by the i-th query
 * block of the group], physical_block = (b / blocks_per_segment) * heads * blocks_per_segment + head * blocks_per_segment + b %
 * blocks_per_segment (the block's position in the all-gathered K / V^T buffers; one segment = the whole sequence on one GPU).
 * lists int32 [heads][ceil(n_q / g)][max_entries], counts int32 [heads][ceil(n_q / g)]; max_entries >= min(g * n_sel, n_k).  Equal
 * scores at the n_sel-th place are taken by ascending block index.  sel_mask (NULL or uint32 [heads][n_q][ceil(n_k / 32)]): bit b of a row
 * = key block b selected by that query block (read back by tests).  n_k <= 2048. */
int wf_bsa_topk_lists(const void* scores, int64_t ld, int heads, int n_q, int n_k, int n_sel, int block, int blocks_per_segment,
                      int* lists, int* counts, int max_entries, uint32_t* sel_mask, void* stream);
/* The cdf selection rule (BSA:226-263, get_select_indices_cdf / get_select_indices_cdf_topk) with the same list building: per query
 * block, the key blocks in descending order of softmax(score / sqrt(128)) as long as their cumulative weight stays <= cdf_threshold
 * (`searchsorted(cdf, threshold, right=True)`: possibly none), at least n_min of them (int((1 - sparsity) * n_k) of the _topk form, 0
 * otherwise).  row_counts int32 [heads][n_q] receives the per-row counts; lists / counts / sel_mask as wf_bsa_topk_lists with
 * max_entries >= n_k.  The chain is evaluated as eager torch evaluates it on the reference's bf16 score tensor -- bf16(score * scale),
 * softmax rounded to bf16, running fp32 sum of the sorted weights rounded to bf16 per element, compared with float32(cdf_threshold) --
 * pinned by tests/golden/g14c_bsa_cdf_bf16.npz (recorded from the reference's function).  Deterministic; for thresholds <= 0.97 the
 * tree scan equals the sequential cumsum exactly, what can differ from a torch run is one bf16 ulp of a weight where exp / the row sum
 * round differently (about one row in a thousand changes its count by one). */
int wf_bsa_cdf_lists(const void* scores, int64_t ld, int heads, int n_q, int n_k, float cdf_threshold, int n_min, int block,
                     int blocks_per_segment, int* lists, int* counts, int max_entries, uint32_t* sel_mask, int* row_counts, void* stream);
/* out[i][:C] = in[index[i]][:C], bf16 rows (16-byte chunks): the two token permutes of BSA:600-610 the refine pass needs per forward
 * (patch tokens into 3D-block order, velocity rows back). */
int wf_gather_rows_bf16(const void* in, int64_t ld_in, const int* index, void* out, int64_t ld_out, int n_rows, int C, void* stream);
/* The sparse attention of BSA:538-560 (flash_attn_bsa_varlen_mask.py:174-285): Q [H][Lq][128], K [H][Lkp][128], Vt [H][Lkp/64][128][64]
 * in 3D-block token order, `block` = 128 or 64 tokens per block; every query block attends to its selected key blocks only.  The
 * selection is given per GROUP of g = 256 / block consecutive query blocks (the 256 query rows of one workgroup): group_lists
 * [H][ceil(Lq/256)][max_entries] int32, entry = physical_block * 2^g + flags (bit i: selected by the i-th query block of the group;
 * physical_block = position of the key block in the K / Vt buffers counted in blocks: ((segment * H + head) * seg_len + offset) / block),
 * the union of the group's lists in any order; group_counts [H][ceil(Lq/256)] entries used.  seg_len = Lkp, or the per-rank shard length
 * when K / Vt are all-gathered shards [P][H][seg_len][128] (as wf_attn_fwd).  O [Lq][ldo] bf16 (block order), head h at columns h*128. */
int wf_attn_bsa_fwd(const void* Q, const void* K, const void* Vt, void* O, int H, int Lq, int Lkp, int seg_len, int ldo,
                    float softmax_scale, const int* group_lists, const int* group_counts, int max_entries, int block, void* stream);

/* ---- UMT5 text encoder (csrc/t5.hip; HF = transformers/models/umt5/modeling_umt5.py, the class RUN:203-204 / PIPE:21 load as
 *      UMT5EncoderModel; worldforge_amd/umt5.py is the host).  The encoder's linears are wf_gemm_bf16; its residual stream is fp32. ---- */
/* UMT5Attention.forward of an encoder layer (HF: scores = q k^T with NO 1/sqrt(d) factor, + position_bias (compute_bias: the layer's own
 * relative_attention_bias embedding at _relative_position_bucket(key - query)) + the extended attention mask, softmax in fp32, P . V):
 *   s[h][i][j] = q_i . k_j + bias[h * num_buckets + bucket_lut[j - i + (lmax - 1)]],  j < kv_len;  O = softmax_j(s) V.
 * Q, K, V bf16 [L, ldqkv] with head h at columns h*64 (three column slices of one stacked QKV GEMM output; ldqkv % 8 == 0, 16-byte
 * aligned), O bf16 [L, ldo] (ldo % 4 == 0, 8-byte aligned), bias f32 [H][num_buckets], bucket_lut uint8 [2 * lmax - 1] (built once by the
 * host from the bidirectional bucket rule; a byte >= num_buckets is read as num_buckets - 1).  Keys j >= kv_len do not exist (HF adds
 * finfo.min to their scores: the same for kv_len >= 1) and their K / V rows are never read; ALL L query rows are computed, the pad rows
 * included, as HF returns them.  Softmax in fp32 with the exact row maximum, P rounded once to bf16, both products on bf16 MFMA with fp32
 * accumulation, the row sum of the un-rounded p in fp32, one rounding of the output.  WF_EINVAL before any device work unless
 * 1 <= kv_len <= L <= min(512, lmax), H >= 1, 1 <= num_buckets <= 256. */
int wf_t5_attn_fwd(const void* Q, const void* K, const void* V, int ldqkv, void* O, int ldo, const float* bias, const void* bucket_lut,
                   int lmax, int num_buckets, int H, int L, int kv_len, void* stream);
/* UMT5DenseGatedActDense's gate (HF: hidden_gelu = gelu_new(wi_0(x)); hidden_linear = wi_1(x); hidden_gelu * hidden_linear): in f32
 * [M, ld] with wi_0 x in columns [0, F) and wi_1 x in [F, 2F) -- ONE wf_gemm_bf16 over the stacked [wi_0; wi_1] weight with WF_EPI_F32 --
 * -> out bf16 [M, F] = rn_bf16(0.5 g (1 + tanh(sqrt(2/pi) (g + 0.044715 g^3))) * u), rounded once; finite for every finite g, u whose
 * product is (|g| up to 1e4 and beyond: tanh saturates).  F % 4 == 0, ld % 4 == 0. */
int wf_t5_gated_gelu(const float* in, int64_t ld, void* out, int M, int F, void* stream);
/* UMT5LayerNorm (HF: variance = x.float().pow(2).mean(-1); x * rsqrt(variance + eps) * weight; no mean subtraction, no bias): x f32
 * [L, C] -> out bf16 [L, C], one rounding; the sum of squares in fp32 in a fixed order.  weight f32 [C]; C % 4 == 0.  (wf_rms_silu_cl
 * is F.normalize with a clamp on the norm, wf_rmsnorm_heads reads bf16 and writes head-major: neither has this contract.) */
int wf_t5_rmsnorm(const float* x, const float* weight, void* out, int L, int C, float eps, void* stream);
/* shared / encoder.embed_tokens (HF: inputs_embeds = self.embed_tokens(input_ids)): ids int32 [L], table bf16 [V, C] -> out f32 [L, C],
 * exact.  The host refuses ids outside [0, V) (ValueError) before the call; the kernel clamps and never reads outside the table. */
int wf_t5_embed(const int* ids, const void* table, float* out, int L, int V, int C, void* stream);

/* ---- CLIP vision encoder (csrc/clip.hip; HF transformers/models/clip/modeling_clip.py: CLIPVisionModel, which the reference loads in
 *      float32; worldforge_amd/clip.py is the host).  Everything is fp32 on the fp32-input MFMA (v_mfma_f32_32x32x2_f32): no operand and no
 *      partial result is narrower than fp32.  The LayerNorms are wf_ln_modulate with plus_one = 0 and WF_F32 output. ---- */
#define WF_EPI_F32_GELU 5        /* out f32 = 0.5 v (1 + erf(v / sqrt 2)), v = acc + bias        (hidden_act "gelu") */
#define WF_EPI_F32_QUICK_GELU 6  /* out f32 = v * sigmoid(1.702 v)                                (hidden_act "quick_gelu") */
/* out[M,N] = epi(X[M,K] . W[N,K]^T + bias), every operand fp32 (row strides ldx, ldw, ldo in elements), each dot product a chain of fp32
 * fma in a fixed order that depends on K alone: two calls give the same bits, no atomics.  epilogue WF_EPI_F32, WF_EPI_F32_ACC (out +=),
 * WF_EPI_F32_GELU or WF_EPI_F32_QUICK_GELU; bias f32 [N] or NULL.  Any M >= 1; K % 4 == 0, N % 4 == 0, leading dimensions % 4, 16-byte
 * aligned pointers; anything else returns WF_EINVAL before any device work. */
int wf_gemm_f32(const float* X, const float* W, const float* bias, float* out, int M, int N, int K, int ldx, int ldw, int ldo, int epilogue,
                void* stream);
/* CLIPAttention.forward without a mask: O = softmax_j(scale * q_i . k_j) V per head, fp32 in and out.  Q, K, V are three column slices of
 * one stacked [L, ldqkv] buffer with head h at columns h * D; O [L, ldo].  The scores, the exact row maximum, p = exp(s - max), the row sum
 * and both products are fp32 (p is never rounded below fp32); the output is acc / sum.  Two calls give the same bits.  WF_EINVAL before
 * any device work unless D % 8 == 0, 8 <= D <= 128, 1 <= L <= 1024, 1 <= H <= 65535, ldqkv % 4 == 0, ldo % 4 == 0, both >= H * D, scale
 * positive and finite, 16-byte aligned pointers. */
int wf_clip_attn_fwd(const float* Q, const float* K, const float* V, int ldqkv, float* O, int ldo, int H, int L, int D, float scale,
                     void* stream);
/* CLIPVisionEmbeddings.patch_embedding (a Conv2d with kernel = stride = p and no bias) as a GEMM operand: pixels f32 [3][S][S] -> rows f32
 * [G * G][3 * p * p], G = S / p, row py * G + px, column c * p * p + ph * p + pw (the flattening order of the conv weight): a copy, exact. */
int wf_clip_patch_rows(const float* pixels, float* rows, int S, int p, void* stream);

/* ---- VGGT front-end (csrc/vit.hip; vggt/models/aggregator.py, vggt/layers/attention.py, rope.py; worldforge_amd/vggt.py is the host): the
 *      DINOv2 backbone and the frame / global blocks run on wf_gemm_bf16 with an fp32 residual stream (what bf16 autocast leaves). ---- */
/* Attention.forward's F.scaled_dot_product_attention without a mask (attention.py:50-72): O = softmax_j(scale * q_i . k_j) V for nseq
 * independent sequences of L tokens, H heads of 64 channels, bf16.  Q, K, V are three column slices of one stacked [nseq * L, ldqkv] buffer
 * (head h at columns h * 64; ldqkv % 8 == 0, 16-byte aligned), O bf16 [nseq * L, ldo] (ldo % 4 == 0, 8-byte aligned); sequence s is rows
 * s * L .. s * L + L - 1 and no row of another sequence is read.  Any L >= 1: the keys stream through LDS in 64-key tiles with an online
 * softmax, the last tile masked inside the kernel.  Scores, running maximum, p and the row sum (of the un-rounded p) are fp32, P is rounded
 * once to bf16, both products are bf16 MFMA with fp32 accumulation, one rounding of the output.  No atomics: two calls give the same bits.
 * WF_EINVAL before any device work unless 1 <= nseq, H <= 65535, L >= 1, nseq * L < 2^31, scale positive and finite. */
int wf_vit_attn_fwd(const void* Q, const void* K, const void* V, int ldqkv, void* O, int ldo, int nseq, int H, int L, float scale,
                    void* stream);
/* q_norm / k_norm and the 2D RoPE (attention.py:54-58, rope.py:133-188), in place on the q and k slices of the stacked bf16 buffer
 * [nseq * L, ldqkv] (head h at columns h * 64; the v slice is not touched).  Per row and head: LayerNorm over the 64 channels (f32 weight /
 * bias [64] per slice, eps), then channels 0..31 rotated by the token's y position and 32..63 by its x position, each half pairing
 * (i, i + 16) with 16 frequencies: out[i] = x[i] cos - x[i+16] sin, out[i+16] = x[i+16] cos + x[i] sin.  cos / sin f32 [max_pos + 1][16],
 * pos int32 [L][2] = (y, x) of the token inside its sequence (aggregator.py:223-228: special tokens (0, 0) = the identity, patch (y, x)
 * carries (y + 1, x + 1)); a position outside 0..max_pos is clamped.  fp32 arithmetic, one rounding; q is multiplied by out_scale in front
 * of the rounding (1 = none).  All four norm pointers NULL: no LayerNorm; cos, sin, pos NULL: no rotation. */
int wf_vit_qk_norm_rope(void* Q, void* K, int ldqkv, const float* q_weight, const float* q_bias, const float* k_weight,
                        const float* k_bias, float eps, const float* cos_tab, const float* sin_tab, int max_pos, const int* pos,
                        int nseq, int L, int H, float out_scale, void* stream);
/* aggregator.py:201 + PatchEmbed's Conv2d with kernel = stride = 14 as a GEMM operand: images f32 [n][3][H][W] in [0, 1] -> rows bf16
 * [n * (H/14) * (W/14)][592] = rn_bf16((x - mean_c) / std_c) (ResNet statistics, fp32) at column c * 196 + ph * 14 + pw; columns 588..591
 * are zero (wf_gemm_bf16 needs K % 8 == 0: the conv weight is stored [C][592] with the same zero columns).  H, W multiples of 14. */
int wf_vit_patch_rows(const float* images, void* rows, int n, int H, int W, void* stream);

/* ---- VGGT's DPT depth head (csrc/dpt.hip; vggt/heads/dpt_head.py = DPT, head_act.py; worldforge_amd/vggt.py is the host).  The reference
 *      runs the head as an fp32 module outside autocast (run_warp.py:234, models/vggt.py:71-76): everything here is fp32 on the fp32-input
 *      MFMA, activations channels-last f32 [n, H, W, C].  The LayerNorm (DPT:214) is wf_ln_modulate, the 1x1 convolutions (DPT:218, 454,
 *      output_conv2.2's input side) and the two ConvTransposes with kernel = stride (DPT:76-81) are wf_gemm_f32. ---- */
/* nn.Conv2d(Cin, Cout, kernel_size=3, stride, padding=1) (DPT:83-85, 102-113, 328-340, 357-358) with what surrounds it fused:
 *   out[i, y, x, co] = relu_out?( sum_{dy, dx, c} X[i, y stride + dy - 1, x stride + dx - 1, c] w[dy, dx, co, c] + bias[co] + R[i, y, x, co] )
 *   X = relu_in ? max(in, 0) : in (zero outside the image);  R = resid ? (relu_resid ? max(resid, 0) : resid) : 0.
 * relu_in + resid + relu_resid is ResidualConvUnit.forward's second half with its in-place ReLU (DPT:376-386: `out = self.activation(x)`
 * overwrites x, so the skip adds relu(x)); relu_out is output_conv2's ReLU (DPT:111).
 * in f32 [n, Hi, Wi, Cin]; w_packed f32 [3][3][Cout][Cin] = weight.permute(2, 3, 0, 1) of the module's [Cout][Cin][3][3]; bias f32 [Cout] or
 * NULL; resid f32 [n, Ho, Wo, Cout] or NULL; out f32 [n, Ho, Wo, Cout], Ho = (Hi - 1) / stride + 1, Wo = (Wi - 1) / stride + 1; out may be
 * neither in nor w_packed (it may be resid: an element is read and written by the same lane).  Every output element is ONE chain of fp32 fma
 * over taps (dy, dx) outer and channels inner, both ascending, then + bias, + R: its bits depend neither on n nor on the tiling; no atomics,
 * two calls give the same bits.  WF_EINVAL before any device work unless n, Hi, Wi >= 1, Cin % 4 == 0, Cout % 4 == 0 (both >= 4), stride 1
 * or 2, in / w_packed / out non-NULL, relu_resid only with resid, every pointer 16-byte aligned, every tensor below 2^31 elements. */
int wf_conv2d_f32(const float* in, const float* w_packed, const float* bias, const float* resid, float* out, int n, int Hi, int Wi, int Cin,
                  int Cout, int stride, int relu_in, int relu_resid, int relu_out, void* stream);
/* custom_interpolate(mode="bilinear", align_corners=True) (DPT:229-234, 453, 459-484) on channels-last maps, in f32 [n, Hi, Wi, C] -> out
 * f32 [n, Ho, Wo, C], as PyTorch evaluates it in fp32: scale = (in - 1) / (out - 1) (0 when out == 1), src = scale * dst, i0 = (int)src,
 * i1 = min(i0 + 1, in - 1), l1 = src - i0, l0 = 1 - l1, out = ly0 (lx0 v00 + lx1 v01) + ly1 (lx0 v10 + lx1 v11).  Equal sizes: an exact copy.
 * _apply_pos_embed (DPT:249-259) fused: col_table f32 [Wo][C / 2] is added to channels 0 .. C/2 - 1 and row_table f32 [Ho][C / 2] to
 * channels C/2 .. C - 1 of the result; both NULL: none.  WF_EINVAL before any device work unless n and every size >= 1, C % 4 == 0, in / out
 * non-NULL and 16-byte aligned, the tables both given or both NULL and 4-byte aligned.  out must not overlap in. */
int wf_resize_bilinear_cl_f32(const float* in, float* out, int n, int Hi, int Wi, int Ho, int Wo, int C, const float* col_table,
                              const float* row_table, void* stream);
/* output_conv2.2 (1x1, Cin -> 2; DPT:112) + activate_head(activation="exp", conf_activation="expp1") (head_act.py): rows f32 [npix, Cin],
 * w f32 [2][Cin], b f32 [2] -> depth f32 [npix] = expf(v0), conf f32 [npix] = 1 + expf(v1), v_j = b[j] + sum_c rows[c] w[j][c] as an fp32 fma
 * chain over ascending c.  No other activation is built.  WF_EINVAL before any device work unless npix >= 1, Cin % 4 == 0, no pointer NULL,
 * rows / w 16-byte aligned, b / depth / conf 4-byte aligned. */
int wf_dpt_depth_out(const float* rows, const float* w, const float* b, float* depth, float* conf, size_t npix, int Cin, void* stream);

/* ---- 3D causal VAE (wan/modules/vae.py; the in-tree statement of diffusers' AutoencoderKLWan), channels-last ----------- */
/* CausalConv3d / Conv2d as implicit GEMM on MFMA (vae.py:17-36, 76-96, 186-220).  in bf16 [Ti,Hi,Wi,Cin] (Cin % 32 == 0),
 * w bf16 [Cout][kt*kh*kw][Cin], bias f32; out (f32 and/or bf16) [To,Ho,Wo,Cout] (+ resid f32 of the same shape).
 *   out[t,y,x] = sum_taps in[t*st+dt-pt, y*ss+dy-ph, x*ss+dx-pw] . w[tap]   (zero outside the input; ph may be negative when
 *   the input is a row slab that already carries its halo rows -- multi-GPU row sharding)
 * up2: read the input through a nearest-exact 2x spatial upsample (vae.py:78);  tsplit: 'upsample3d' frame interleave
 * (vae.py:134-137): output frame t, channel half h -> frame 1 + 2t + h of a [1+2*To, Ho, Wo, Cout/2] tensor.
 * zero_page: >= 16 bytes of zeros in device memory (enables the DMA-gather ping-pong kernel for large stride-1 layers) or NULL. */
int wf_conv3d_cl(const void* in, const void* w, const float* bias, const float* resid, float* out_f32, void* out_bf16, int Ti,
                 int Hi, int Wi, int Cin, int To, int Ho, int Wo, int Cout, int kt, int kh, int kw, int st, int ss, int pt, int ph,
                 int pw, int up2, int tsplit, const void* zero_page, void* stream);
/* wf_conv3d_cl whose output pixel (t, y, x) of the [To, Ho, Wo] grid lands at pixel (t, sy * y + oy, sx * x + ox) of a [To, out_H, out_W]
 * tensor (resid, if given, is read at the same place).  Lets the nearest-2x upsample + 3 x 3 convolution of Resample (vae.py:76-86) run as
 * its four phases: output (2 y + py, 2 x + px) only ever sees source rows {y - 1 + py, y + py} and columns {x - 1 + px, x + px}, with the
 * 3 x 3 taps that fall on the same source pixel summed beforehand -- 2 x 2 convolutions on the source grid, 4 / 9 of the multiply-adds. */
int wf_conv3d_cl_scatter(const void* in, const void* w, const float* bias, const float* resid, float* out_f32, void* out_bf16, int Ti, int Hi,
                         int Wi, int Cin, int To, int Ho, int Wo, int Cout, int kt, int kh, int kw, int st, int ss, int pt, int ph, int pw,
                         const void* zero_page, int out_H, int out_W, int sy, int oy, int sx, int ox, void* stream);
/* The FLOP-heavy layers (3x3x3, stride 1, causal: every ResidualBlock conv, vae.py:186-220) with the input patch resident in LDS:
 * an 8 x 64 pixel tile of one output frame x 96 output channels per workgroup, all 27 taps read the (3 x 10 x 66)-pixel patch of a
 * 16-channel slice from LDS.  Weights in the re-packed layout [27][Cin/16][Cout][16] produced by wf_conv3d_pack333 from
 * [Cout][27][Cin].  in [T,Hi,Wi,Cin] bf16 (Hi = Ho for ph = 1; row slabs carry their halo rows: Hi = Ho + 2, ph = 0),
 * out [T,Ho,Wi,Cout]; Cin % 32 == 0, Cout % 32 == 0.  zero_page: zeros, zero_page_bytes >= wf_conv3d_333_zero_page_bytes(Wi, Cin_stored,
 * layout) of them -- the lanes that stage padding pixels read it at the same wave-uniform slice offset the other lanes read the input at
 * (one 64-bit add per LDS-DMA piece instead of a per-lane select).  Same arithmetic as wf_conv3d_cl.
 * layout 0: in is pixel-major [T,Hi,Wi,Cin_stored]; layout 1: slice-major [T,Hi,Cin_stored/16,Wi,16] (what wf_rms_silu_cl_blocked
 * writes: a patch row of a 16-channel slice is contiguous, so the LDS-DMA gather reads whole cache lines).  Cin_stored = Cin, or
 * 2/3 Cin when the fp32-class three-term operand [hi | lo | hi] (wf_split_bf16x3 side 0) is stored as [hi | lo] and its hi half is
 * read for both K thirds. */
int wf_conv3d_pack333(const void* w, void* w_packed, int Cout, int Cin, void* stream);
size_t wf_conv3d_333_zero_page_bytes(int Wi, int Cin_stored, int layout);
int wf_conv3d_333(const void* in, const void* w_packed, const float* bias, const float* resid, float* out_f32, void* out_bf16, int T,
                  int Hi, int Wi, int Cin, int Ho, int Cout, int ph, const void* zero_page, size_t zero_page_bytes, int layout,
                  int Cin_stored, void* stream);
/* Direct convolution for the thin layers (3->96, 16->384, 96->3, 384->32, 1x1x1 quant convs; vae.py:288, 316, 392, 421, 505-506).
 * in f32 or bf16 channels-last, w f32 [taps][Cin][Cout]; clamp > 0 clamps the output (autoencoder_kl_wan.py:1222). */
int wf_conv3d_small(const void* in, int in_dtype, const float* w, const float* bias, float* out_f32, void* out_bf16, int Ti, int Hi,
                    int Wi, int Cin, int To, int Ho, int Wo, int Cout, int kt, int kh, int kw, int st, int ss, int pt, int ps,
                    float clamp, void* stream);
/* RMS_norm over channels (vae.py:39-54) [+ SiLU]: x f32 [npix, C] -> bf16 and/or f32. */
int wf_rms_silu_cl(const float* x, const float* gamma, void* out_bf16, float* out_f32, size_t npix, int C, int silu, void* stream);
/* Row softmax of the mid-block attention scores (vae.py:252-256): P[m, :N] = softmax(S[m, :N] * scale), P[m, N:ldp] = 0. */
int wf_softmax_rows(const float* S, int lds, void* P, int ldp, int M, int N, float scale, void* stream);
/* bf16 in [R, ld_in] (first C columns) -> out [C, ld_out], columns R..ld_out zero. */
int wf_transpose_bf16(const void* in, int ld_in, void* out, int ld_out, int R, int C, void* stream);
/* fp32-class VAE (the reference loads the VAE with torch_dtype=torch.float32, infer_worldforge.py:185-189; every conv / linear of
 * vae.py then contracts fp32 operands).  The matrix cores take bf16, so an fp32 operand x is carried as hi = bf16(x), lo = bf16(x - hi)
 * and a contraction as hi.hi + lo.hi + hi.lo in fp32 accumulators (dropped: lo.lo <= 2^-16 relative, tails <= 2^-17): src f32
 * [rows, C] (row stride ld_src) -> dst bf16 [rows, 3C] (row stride ld_dst); side 0 (activation) = [hi | lo | hi], side 1 (weight) =
 * [hi | hi | lo]: the unchanged conv / GEMM kernels then run on 3C "channels". */
int wf_split_bf16x3(const float* src, int64_t ld_src, void* dst, int64_t ld_dst, size_t rows, int C, int side, void* stream);
/* wf_rms_silu_cl with the side-0 three-term output ([npix, 3C] bf16) written directly. */
int wf_rms_silu_cl_x3(const float* x, const float* gamma, void* out_x3, size_t npix, int C, int silu, void* stream);
/* wf_rms_silu_cl writing the slice-major conv operand of wf_conv3d_333 (layout 1): x f32 [npix, C] (npix = whole rows of W pixels)
 * -> bf16 [npix / W][C/16][W][16]; split != 0: the fp32-class operand stored as [hi | lo] slices, [npix / W][2C/16][W][16].
 * halo_rows = Hs > 0 (row slabs of the sharded VAE, x = [T][Hs][W][C]): the output is the halo-padded operand [T][Hs + 2][...] and row
 * (t, y) is written to (t, y + 1); the two halo rows of every frame are left to the caller (neighbours' rows / zeros). */
int wf_rms_silu_cl_blocked(const float* x, const float* gamma, void* out, size_t npix, int C, int silu, int W, int split, int halo_rows,
                           void* stream);
/* wf_softmax_rows with f32 probabilities (vae.py:252-256 in fp32) / wf_transpose_bf16 on f32. */
int wf_softmax_rows_f32(const float* S, int lds, float* P, int ldp, int M, int N, float scale, void* stream);
int wf_transpose_f32(const float* in, int ld_in, float* out, int ld_out, int R, int C, void* stream);
/* ---- fp16 operand formats of the VAE (round 4) -----------------------------------------------------------------------------------------
 * The reference's VAE is fp32 (infer_worldforge.py:185-189).  The three-term split above on BF16 parts (8-bit significands) leaves
 * ~2^-16 per product; the same split on FP16 parts (11-bit significands: hi = fp16(x), lo = fp16(x - hi), contraction hi.hi + lo.hi +
 * hi.lo on v_mfma_f32_32x32x16_f16, same rate) leaves ~2^-22 -- two decimal digits closer to IEEE fp32 at the same cost; it is the
 * VAE's default ("fp16x3").  fp16 has a 5-bit exponent: values beyond +-65504 do not fit.  The producers raise a sticky flag
 * (wf_f16_overflow_flag) that the host turns into an error; the bf16 split ("bf16x3") remains for such weights.
 * Every *_f16 entry point is its bf16 namesake with fp16 in place of bf16 in the operands (and in a 16-bit output copy).
 * acc_scale (round 5): `lo = fp16(x - hi)` is an fp16 SUBNORMAL for |x| < 2^-3 (absolute floor 2^-25), so a weight of
 * 0.02 was carried to ~2^-18 relative, not 2^-22.  The host therefore stores every weight matrix multiplied by an exact power of two 2^k
 * (its largest magnitude lands in [2^13, 2^14): lo is a normal fp16 for every weight above 2^-17 of the layer's largest) and passes
 * acc_scale = 2^-k: the kernels compute out = acc * acc_scale + bias (+ residual) -- exact, one fma in place of the add. */
int wf_split_f16x3(const float* src, int64_t ld_src, void* dst, int64_t ld_dst, size_t rows, int C, int side, void* stream);
int wf_rms_silu_cl_x3_f16(const float* x, const float* gamma, void* out_x3, size_t npix, int C, int silu, void* stream);
int wf_rms_silu_cl_blocked_f16(const float* x, const float* gamma, void* out, size_t npix, int C, int silu, int W, int split,
                               int halo_rows, void* stream);
int wf_conv3d_cl_f16(const void* in, const void* w, const float* bias, const float* resid, float* out_f32, void* out_f16, int Ti,
                     int Hi, int Wi, int Cin, int To, int Ho, int Wo, int Cout, int kt, int kh, int kw, int st, int ss, int pt, int ph,
                     int pw, int up2, int tsplit, const void* zero_page, float acc_scale, void* stream);
int wf_conv3d_cl_scatter_f16(const void* in, const void* w, const float* bias, const float* resid, float* out_f32, void* out_f16, int Ti,
                             int Hi, int Wi, int Cin, int To, int Ho, int Wo, int Cout, int kt, int kh, int kw, int st, int ss, int pt,
                             int ph, int pw, const void* zero_page, int out_H, int out_W, int sy, int oy, int sx, int ox, float acc_scale,
                             void* stream);
int wf_conv3d_333_f16(const void* in, const void* w_packed, const float* bias, const float* resid, float* out_f32, void* out_f16, int T,
                      int Hi, int Wi, int Cin, int Ho, int Cout, int ph, const void* zero_page, size_t zero_page_bytes, int layout,
                      int Cin_stored, float acc_scale, void* stream);
/* *out = 1 if a producer converted a value beyond the fp16 range (or a NaN) since the last reset; synchronises `stream`. */
int wf_f16_overflow_flag(int* out, int reset, void* stream);
/* The same word copied asynchronously into page-locked host memory behind the work queued on `stream` so far: no synchronisation (the
 * caller records an event behind the call and reads the word once it has fired) -- what AutoencoderKLWan.encode / decode use since
 * round 5, so that a VAE call never stalls the host (SURVEY 8b "no hidden device syncs"). */
int wf_f16_overflow_flag_async(int* pinned_host_out, void* stream);
/* [C, N] f32 -> [N, Cpad] (f32 and/or bf16; channels C..Cpad zero, so thin inputs fill an MFMA K slice);
 * [N, ld] f32 (first C channels) -> [C, N] f32 with optional clamp (autoencoder_kl_wan.py:1222).  N = T*H*W. */
int wf_ncthw_to_cl(const float* in, float* out_f32, void* out_bf16, int C, int Cpad, size_t N, void* stream);
int wf_cl_to_ncthw(const float* in, float* out, int C, int ld, size_t N, float clamp, void* stream);
/* ---- the one-term fp16 operand format of the VAE ("fp16", round 6) -------------------------------------------------------------------
 * What an fp32 convolution keeps of its operands when TF32 is allowed: cuDNN fp32 convolutions are TF32-eligible under PyTorch's
 * defaults (torch.backends.cudnn.allow_tf32 = True; the LongCat entry also sets it explicitly, run_longcat_worldforge_single.py:144-146),
 * i.e. 10 explicit mantissa bits per multiplicand and fp32 accumulation.  fp16 has the same 10 explicit bits: the one-term mode feeds
 * hi = fp16(x) alone to the *_f16 conv / GEMM kernels above (weights stored power-of-two scaled, acc_scale epilogue, range flag) at one
 * third of the three-term mode's matrix work.  These are the producers of that operand; every one raises the range flag of
 * wf_f16_overflow_flag.  wf_cast_f16: src f32 [rows, C] (row stride ld_src) -> dst fp16 [rows, C] (row stride ld_dst), C and the strides
 * multiples of 4.  The others are their bf16 namesakes with an fp16 16-bit output. */
int wf_cast_f16(const float* src, int64_t ld_src, void* dst, int64_t ld_dst, size_t rows, int C, void* stream);
/* Any of the operand producers (fmt 0: wf_split_bf16x3, 1: wf_split_f16x3, 2: wf_cast_f16, 3: plain bf16 rounding) writing straight into a
 * halo-padded destination -- the row slabs of the sharded VAE, [T][Hs + 2][W][..] with the slab's own rows at 1 .. Hs of every frame: source
 * row r -> destination row lead_rows + r + (r / group_rows) * gap_rows (group_rows = Hs W, gap_rows = 2 W, lead_rows = W; group_rows = 0: no
 * gaps).  Same values as the stand-alone producers: it replaces producer + copy (worldforge_amd/vae.py _halo_pad_of). */
int wf_operand_rows(const float* src, int64_t ld_src, void* dst, int64_t ld_dst, size_t rows, int C, int fmt, int side, size_t group_rows,
                    size_t gap_rows, size_t lead_rows, void* stream);
int wf_rms_silu_cl_f16(const float* x, const float* gamma, void* out_f16, float* out_f32, size_t npix, int C, int silu, void* stream);
int wf_softmax_rows_f16(const float* S, int lds, void* P, int ldp, int M, int N, float scale, void* stream);
int wf_ncthw_to_cl_f16(const float* in, float* out_f32, void* out_f16, int C, int Cpad, size_t N, void* stream);

/* ---- stage-1 forward warping (vggt/modules/utils_warp.py:863-945, warp_single_img without crack filling) ------------------------- */
/* Depth-guided forward splat of one image to n_cameras new views: un-project (fp64) -> world -> each camera -> project -> nearest pixel,
 * nearest source wins (z-buffer).  image f32 [H][W][3] in [0,1]; depth f32 [H][W] (NaN / <= 0 = invalid, i.e. already filtered by
 * confidence); geometry = 30 doubles {K^-1 (9), K (9), R^T (9), -R^T t (3)} of the source camera; cameras = n x 12 doubles (rows of
 * [R | t] of every new camera).  out_images u8 [n][H][W][3], out_masks u8 [n][H][W] (1 = written), out_depth f32 [n][H][W] (NaN =
 * empty); zbuffer: 12 * n*H*W bytes of scratch, 8-byte aligned (a 64-bit depth key and a 32-bit owner word per target pixel).  Where
 * several sources reach a target pixel with bit-equal z, the one with the lowest raster index y * W + x writes it. */
int wf_warp_splat(const float* image, const float* depth, const double* geometry, const double* cameras, void* out_images, void* out_masks,
                  float* out_depth, void* zbuffer, int n_cameras, int H, int W, void* stream);
/* Depth-aware crack filling of the warped views (vggt/modules/utils_warp.py depth_aware_crack_filling :647-691 with segment_depth_map
 * :506-536, fill_segment_cracks :567-634 (fast outlier test), fill_small_cracks step 1 :390-430, vectorized_depth_estimation :539-564,
 * merge_depth_segments :637-676, as warp_single_img runs them per view :954-985): img u8 [n,H,W,3], mask u8 [n,H,W], depth f32 [n,H,W]
 * (NaN = empty) -> filled image / mask / depth of the same shapes.  min_neighbors: outlier threshold (3 x 3 count incl. the centre);
 * min_valid_neighbors: valid 8-neighbours a newly covered pixel needs; num_segments <= 5.  OpenCV's filter2D / morphologyEx are restated
 * (BORDER_REFLECT_101 correlation; closing that ignores the border): parity with a real cv2 is unpinned.  workspace:
 * wf_crack_fill_workspace_bytes(n, H, W) bytes. */
size_t wf_crack_fill_workspace_bytes(int n, int H, int W);
int wf_crack_fill(const void* img, const void* mask, const float* depth, void* out_img, void* out_mask, float* out_depth, int n, int H,
                  int W, int min_neighbors, int min_valid_neighbors, int num_segments, void* workspace, void* stream);
/* The same filling with the two parameters that run_warp.py ships and wf_crack_fill fixes: neighbor_radius 1..4 (the outlier test counts
 * the pixels of the pixel's OWN segment in the (2 r + 1)^2 window, centre included, BORDER_REFLECT_101, utils_warp.py:577-588) and
 * num_segments 1..16.  Everything after the outlier test is 3 x 3 as in wf_crack_fill; at (radius 1, <= 5 segments) the two agree bit for
 * bit.  Refused: H <= radius or W <= radius (reflect-101 is undefined there), a radius or a segment count out of range.  The per-segment
 * depth sums that order the merge are reduced in a fixed tree (no floating-point atomics).  workspace:
 * wf_crack_fill_ex_workspace_bytes(n, H, W) bytes, no initialisation needed. */
size_t wf_crack_fill_ex_workspace_bytes(int n, int H, int W);
int wf_crack_fill_ex(const void* img, const void* mask, const float* depth, void* out_img, void* out_mask, float* out_depth, int n, int H,
                     int W, int min_neighbors, int min_valid_neighbors, int num_segments, int neighbor_radius, void* workspace,
                     void* stream);

/* The confidence filter of warp_single_img (vggt/modules/utils_warp.py:784-808).
 * wf_select_pair_f32: exact selection on n fp32 values (device): out = 12 device bytes {the k-th smallest (0-based), the min(k + 1, n - 1)-th
 * smallest, the number of NaNs as a u32}; a NaN sorts last, as in numpy.  Radix select on a monotone unsigned key with integer
 * histograms: the same input gives the same bits.  The host turns the pair into np.percentile's "linear" threshold.
 * wf_depth_conf_filter: depth, conf f32 [n] -> out_depth f32 [n] and out_stats = 2 device doubles {mean, count} of the pixels the
 * reference averages; the mean is a fixed-order fp64 reduction (NaN when the count is 0).  mode 0: out = conf > threshold ? depth : NaN,
 * mean over the kept non-NaN depths (<= 0 included, as np.nanmean); mode 1 (conf_threshold == 1.0): out = depth, mean over the depths
 * that are not NaN and > 0; mode 2 (no confidence map, conf may be NULL): out = NaN unless the depth is not NaN and > 0, mean over those. */
size_t wf_select_pair_f32_workspace_bytes(void);
int wf_select_pair_f32(const float* x, int64_t n, int64_t k, void* out, void* workspace, void* stream);
size_t wf_depth_conf_filter_workspace_bytes(void);
int wf_depth_conf_filter(const float* depth, const float* conf, float threshold, int mode, float* out_depth, double* out_stats, int64_t n,
                         void* workspace, void* stream);

/* fill_small_cracks in full (vggt/modules/utils_warp.py:386-455) -- what warp_single_img runs INSTEAD of the depth-aware filling for a view
 * with <= 100 splatted depths (:957-962, 973-981): step 1 = 3 x 3 closing + mean of the valid 8-neighbours (>= min_valid_neighbors of them);
 * step 2 (has_depth_conf != 0 and step 1 filled fewer than half of the holes) = the 4-connected hole components of <= min(max_crack_size, 4)
 * pixels in scipy.ndimage.label order, pixel by pixel, from the valid 3 x 3 neighbours whose original_depth (the SOURCE view's map, indexed at
 * the target pixel as the reference does) is within depth_threshold of the pixel's -- sequential, one lane.  One view: img u8 [H][W][3],
 * mask u8 [H][W], original_depth f32 [H][W] (may be NULL when has_depth_conf == 0) -> out_img u8, out_mask u8.  The image is float32 (u8 / 255)
 * through both steps and quantised once ((x * 255) truncated), as the reference.  workspace: wf_fill_small_cracks_workspace_bytes(H, W). */
size_t wf_fill_small_cracks_workspace_bytes(int H, int W);
int wf_fill_small_cracks(const void* img, const void* mask, const float* original_depth, int has_depth_conf, void* out_img, void* out_mask,
                         int H, int W, float depth_threshold, int max_crack_size, int min_valid_neighbors, void* workspace, void* stream);

/* ---- stage-1 of the dynamic-scene path: DepthCrafter point-cloud renderer (DepthCrafter/utils.py, warp_depthcrafter.py:255-288) ------- */
/* The three entry points below run one set of kernels: wf_points_render and wf_depth_edge_mask are the two halves of wf_dc_warp_frames at
 * T = 1, fed from a stored point array / depth plane instead of the disparity.  Every square window runs as a row and a column pass. */
/* project_points_to_image_pytorch (utils.py:103-171): pytorch3d PointsRasterizer(radius, points_per_pixel = 10) -> idx[..., 0] = the
 * covering point of smallest view depth per pixel -> image = features[idx], mask = idx != -1 -> 5 x 5 opening of the mask (morph) ->
 * image zeroed outside it.  points f32 [n][3] (world), features f32 [n][F], drop (NULL or u8 [n]: 1 = point removed by the edge filter);
 * camera = 16 floats in pytorch3d's convention {R' (9, row-major, view = p R' + T'), T' (3), focal' (2), principal' (2)}, i.e. the result
 * of _cameras_from_opencv_projection for the reference's (extrinsic, K, image size) -- computed by the host (worldforge_amd/warp.py).
 * out_image f32 [H][W][F], out_mask u8 [H][W].  pytorch3d / OpenCV are absent from the reference tree: parity with them is unpinned.
 * The z-buffer key is view depth bits << 32 | point index: the nearest point wins, an exact tie goes to the smaller index. */
size_t wf_points_render_workspace_bytes(int H, int W);
int wf_points_render(const float* points, const float* features, const void* drop, int n, int F, const float* camera, int H, int W,
                     float radius, int morph, float* out_image, void* out_mask, void* workspace, void* stream);
/* filter_edge_points (utils.py:523-567): out_drop u8 [H][W] = dilate_{2 d + 1}(Sobel magnitude / its maximum > edge_threshold) |
 * (max - min of the depth over the (2 r + 1)^2 window > jump_threshold); depth f32 [H][W].  d = edge_dilation, r = neighbor_radius.
 * Borders: the dilation ignores the outside, Sobel reflect-101, jump test scipy "reflect". */
size_t wf_depth_edge_mask_workspace_bytes(int H, int W);
int wf_depth_edge_mask(const float* depth, int H, int W, double edge_threshold, int edge_dilation, float jump_threshold, int neighbor_radius,
                       void* out_drop, void* workspace, void* stream);
/* The whole frame loop of run_warping (DepthCrafter/warp_depthcrafter.py:257-290) for T frames in one call: per frame
 * depth_frame = 1.0f / (disparity + 0.1f) (:259), the point ((j - cx) * z) / fx, ((i - cy) * z) / fy, z (:262-266, never stored), for the
 * frames t >= edge_filter_from the edge filter of wf_depth_edge_mask on depth_frame with that frame's own Sobel maximum (:269-281; the
 * reference passes 1, a value >= T switches the filter off), one z-buffer per frame with wf_points_render's key and tie rule (the point
 * index being the pixel's raster index in its frame), the 5 x 5 opening (morph != 0), image = owner's colour inside the mask, 0 outside (:283-287), and the 8-bit frame cv2.imwrite makes of the float32
 * image (:292-294: convertTo(CV_8U) = the fp32 product x * 255.0f rounded to nearest, ties to even, then saturated; RESTATED and unpinned
 * like the other OpenCV pieces).  The per-frame entry points are this call at T = 1.  No floating-point atomics: the Sobel maxima are
 * integer maxima on the bits of non-negative doubles.
 * frames f32 [T][H][W][3] in [0, 1]; disparity f32 [T][H][W] (the content of depth.npz); cameras f32 [T][16] ON THE DEVICE, each as
 * wf_points_render's camera; fx, fy, cx, cy = K.  out_images u8 [T][H][W][3], out_masks u8 [T][H][W] (0 / 1), out_images_f32 f32
 * [T][H][W][3] or NULL.  Refused (WF_EINVAL): T, H or W <= 0; T > 65535; H or W < 2; H * W >= 2^31; radius outside (0, 0.05]; edge_dilation or
 * neighbor_radius outside 0..15; edge_filter_from < 0.  workspace: wf_dc_warp_frames_workspace_bytes(T, H, W) bytes (11 per pixel), no
 * initialisation needed. */
size_t wf_dc_warp_frames_workspace_bytes(int T, int H, int W);
int wf_dc_warp_frames(const float* frames, const float* disparity, const float* cameras, float fx, float fy, float cx, float cy,
                      double edge_threshold, int edge_dilation, float jump_threshold, int neighbor_radius, int edge_filter_from, float radius,
                      int morph, int T, int H, int W, void* out_images, void* out_masks, float* out_images_f32, void* workspace, void* stream);
/* torchvision.transforms.functional.resize(frames, (H, W)) on a float tensor (warp_depthcrafter.py:203) =
 * torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=antialias != 0), channels-last: in f32 [T][h][w][3] ->
 * out f32 [T][H][W][3], columns first, then rows, each output index with its own weight row.  antialias: scale = in / out, support =
 * max(scale, 1), centre = scale (i + 0.5), taps max(0, int(centre - support + 0.5)) .. min(in, int(centre + support + 0.5)), triangle
 * weights at (j - centre + 0.5) / max(scale, 1), normalised by their sum.  Without: the two taps around scale (i + 0.5) - 0.5 (clamped at
 * 0).  Equal sizes copy the input bits.  workspace: wf_resize_bilinear_aa_f32_workspace_bytes(T, h, w, H, W, antialias) bytes. */
size_t wf_resize_bilinear_aa_f32_workspace_bytes(int T, int h, int w, int H, int W, int antialias);
int wf_resize_bilinear_aa_f32(const float* in, float* out, int T, int h, int w, int H, int W, int antialias, void* workspace, void* stream);
/* PIL.Image.resize on 8-bit images (Pillow's fixed-point resample, modes L and RGB), channels-last: in u8 [T][h][w][C] -> out u8
 * [T][H][W][C], C = 1 or 3.  The caller supplies Pillow's tables per axis (worldforge_amd/resample.py: pil_resample_tables), ON THE DEVICE:
 * bounds i32 [out][2] = (first tap, tap count), coefs i32 [out][k] = the normalised filter weights rounded to 22 fractional bits, zero
 * behind the count.  One output sample is clamp(((1 << 21) + sum_j px[first + j] coefs[j]) >> 22, 0, 255) in int32 (arithmetic shift).
 * Columns first into a u8 [T][h][W][C] intermediate in the workspace, then rows; w == W skips the column pass and h == H the row pass (the
 * skipped pass's tables may be NULL), both equal copy the input.  No floating point, no atomics; the bytes do not depend on the grid.
 * The tables are trusted: every first + count must lie inside its axis (the Python wrapper builds them itself).  Refused (WF_EINVAL):
 * a size <= 0, C not 1 or 3, a null pointer, a pass without its tables or with k <= 0.  workspace: wf_resample_u8_workspace_bytes(...) bytes
 * (NULL allowed when at most one pass runs). */
size_t wf_resample_u8_workspace_bytes(int T, int h, int w, int H, int W, int C);
int wf_resample_u8(const uint8_t* in, uint8_t* out, int T, int h, int w, int H, int W, int C, const int32_t* xbounds, const int32_t* xcoefs,
                   int xk, const int32_t* ybounds, const int32_t* ycoefs, int yk, void* workspace, void* stream);
/* A window of wf_resample_u8's result, looked up and planar, without the frames in between: in u8 [T][h][w][C] (C = 1 or 3) -> out f32
 * [T][C][Hc][Wc] = lut[c][R[t][y0 + i][x0 + j][c]], R = what wf_resample_u8 writes for H x W with the same tables (both passes are
 * independent per pixel, so the window alone is exact).  lut f32 [C][256] and the tables on the device; the tables are the WHOLE axes'
 * (W and H rows) and trusted as for wf_resample_u8, and the row table must be one built for h -> H with taps no further than (yk - 1) / 2
 * from (i + 0.5) h / H, as resample.filter_tables builds it: the column pass covers the source rows such a window can tap (rows outside
 * them are read from the workspace as they lie there).  Column pass (w != W): the window's columns of those rows into a u8 intermediate
 * in the workspace, as Pillow rounds between the passes; then one kernel runs the row taps (int32 sum from 1 << 21, >> 22, clamp), the
 * look-up and the planar store.  w == W: no column pass, the kernel reads `in` at column x0 (workspace may be NULL); h == H: one tap per
 * row; both: a windowed look-up.  The bytes do not depend on the grid.  Refused (WF_EINVAL) before any launch: a size <= 0, C not 1 or
 * 3, a window that leaves H x W, a null in / out / lut, a pass without its tables or with k <= 0, a column pass without the workspace.
 * workspace: wf_resample_u8_window_f32_workspace_bytes(...) bytes (0 for arguments the entry refuses). */
size_t wf_resample_u8_window_f32_workspace_bytes(int T, int h, int w, int H, int W, int C, int y0, int x0, int Hc, int Wc);
int wf_resample_u8_window_f32(const uint8_t* in, float* out, int T, int h, int w, int H, int W, int C, int y0, int x0, int Hc, int Wc,
                              const int32_t* xbounds, const int32_t* xcoefs, int xk, const int32_t* ybounds, const int32_t* ycoefs, int yk,
                              const float* lut, void* workspace, void* stream);
/* 8-bit channels-last frames through a 256-entry table into planar floats: in u8 [T][h][w][C], lut f32 [256] (device) -> out f32
 * [C][T][h][w], out = lut[in].  The table carries the host's own u8 -> f32 expression, so no division runs on the device. */
int wf_u8_lut_planar_f32(const uint8_t* in, const float* lut, float* out, int T, int h, int w, int C, void* stream);

/* ---- measurement aid (bench.py `box_calib_tflops`) -------------------------------------------------------------------------------------
 * One launch of a fixed register-only stream of v_mfma_f32_32x32x16_bf16 (256 workgroups x 4 waves, one per SIMD, 16 accumulator tiles per
 * wave, iters x 16 MFMAs each): what THIS box sustains on the matrix pipe alone under its power limit.  src: 1 MiB of bf16 operand values
 * (N(0,1): the rate depends on the data), sink: >= 4 bytes; *flop (host, may be NULL) receives the launch's flop count.  Asynchronous. */
int wf_calib_mfma(const void* src, float* sink, int iters, double* flop, void* stream);
/* A stream-ordered delay of `us` microseconds (one wave polling the 100 MHz wall clock): the stand-in for a collective's transfer time when
 * one GPU plays one rank of N under a bandwidth model (parallel.LoopbackComm(link model), bench.py --as-rank-of N --emulate-comm). */
int wf_delay_us(double us, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WF_HIP_H_ */
