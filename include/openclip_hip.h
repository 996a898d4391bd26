/*
 * openclip_hip.h -- C ABI of libopenclip_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * CLIP training hot path of mlfoundations/open_clip.
 *
 * The reference has no native code: its device work is a set of ATen / c10d call sites
 * (SURVEY.md 2.3, K1..K14).  Every entry point below names the reference call site it replaces
 * (file:line under /root/reference/src/open_clip).  A reference-side binding is plain ctypes
 * (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain pointers + sizes; the caller owns all memory (device pointers unless stated otherwise);
 *     the library never allocates.
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work on it (async).
 *   - re-entrant, no global device state (the backward pass runs on the autograd thread).  The only process-global state in the
 *     library are the developer knobs of include/openclip_hip_debug.h (kernel selection / ablation switches for experiments:
 *     never needed, never touched by the product path, defaults = the shipped behaviour).
 *   - return 0 on success, negative ocn_status on error; ocn_last_error() holds the message
 *     (thread-local).  Python wrappers turn that into RuntimeError, like the reference's asserts.
 *   - "bf16" buffers are raw 16-bit bfloat16; residual stream, statistics, losses and weight
 *     gradients are fp32.
 */
#ifndef OPENCLIP_HIP_H
#define OPENCLIP_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ocn_stream_t; /* hipStream_t */

enum ocn_status { OCN_OK = 0, OCN_ERR_INVALID = -1, OCN_ERR_LAUNCH = -2, OCN_ERR_UNSUPPORTED = -3 };

/* epilogues of ocn_gemm_nt */
enum ocn_epilogue {
    OCN_EPI_BF16 = 0,           /* out_bf16 = alpha*acc + bias                                            */
    OCN_EPI_BIAS_GELU = 1,      /* out_bf16 = gelu(acc+bias); aux_u8 = gelu'(acc+bias) in 8-bit fixed point (for EPI 3) */
    OCN_EPI_BIAS_RESID_F32 = 2, /* out_f32 = resid_f32 + acc + bias                                       */
    OCN_EPI_DGELU = 3,          /* out_bf16 = acc * decode(aux_u8)   (aux = the gelu' saved by EPI 1)      */
    OCN_EPI_F32 = 4,            /* out_f32 = alpha*acc + bias                                             */
    OCN_EPI_BIAS_QUICKGELU = 7, /* EPI 1 with QuickGELU, x * sigmoid(1.702 x) (layers.py:29-32; `quick_gelu` configs); (9: internal) */
    OCN_EPI_BIAS_RESID_BF16 = 8 /* out_bf16 = bf16(resid_bf16 + bf16(acc + bias)): the residual add on a bf16 stream exactly as the reference's
                                   autocast evaluates it (F.linear's bf16 result, then `q_x + ...` in bf16: transformer.py:328-329) */
};

const char* ocn_last_error(void);
/* ABI version of this header: ocn_version() of the library that is loaded must EQUAL it (open_clip_amd/_lib.py::load and
 * __graft_entry__.build() check; a stale .so behind OCN_LIB_PATH would otherwise receive shifted arguments without any error).
 *   102 (round 5)  ocn_sumsq_multi takes a per-chunk workspace (reproducible sum); ocn_siglip_rows takes the bias as a device value.  BREAKING since 101 and now carried by the number:
 *                  ocn_layernorm_bwd / ocn_embed_assemble_bwd / ocn_token_embed_bwd_sorted[_varlen] / ocn_softmax_ce_rows / ocn_siglip_rows took
 *                  extra arguments in round 4, and the logit-gradient matrix G written by ocn_softmax_ce_rows / ocn_fused_logits_ce /
 *                  ocn_siglip_rows holds softmax (sigmoid) * grad_scale WITHOUT the -onehot term (the caller applies it as an exact rank-1
 *                  update: open_clip_amd/loss.py::_PairTerm.dX / dY). */
/*   103 (round 6)  bf16 residual stream of the image tower: ocn_layernorm_fwd / ocn_layernorm_bwd / ocn_gather_rows take dtype flags, ocn_gemm_nt
 *                  takes `resid` as void* (fp32 or bf16 by epilogue) and knows OCN_EPI_BIAS_RESID_BF16; new: ocn_comm_count, ocn_comm_sendrecv; ocn_fused_logits_ce is ONE
 *                  pass now: G holds exp(logit - shift), the row scale comes back in `rowscale` (new argument); new: ocn_gemm_nt_splitk[_plan],
 *                  ocn_scale_rows_bf16, ocn_sub_scaled_rows.
 *   104 (round 6)  new: ocn_set_tile_rescue / ocn_get_tile_rescue (no signature changed).
 *   105            patch dropout of the image tower: new ocn_patch_keep_plan, ocn_patch_keep_inverse, ocn_patchify_keep, ocn_patchify_u8_keep,
 *                  ocn_embed_assemble_keep_fwd, ocn_embed_assemble_keep_bwd (no signature changed).
 *   106            BREAKING: one entry point per image-embedding op.  ocn_patchify / ocn_patchify_u8 / ocn_embed_assemble_fwd take a nullable `keep` and K,
 *                  ocn_embed_assemble_bwd a nullable `inv` and K; the four `_keep` twins of 105 are gone.
 *   107            CLIPA towers (mean-pooled image tower without ln_pre): new ocn_mean_pool_fwd, ocn_mean_pool_bwd, ocn_cast_bf16_f32 (no signature changed).
 *   108            validation metrics (retrieval ranks, zero-shot top-k): new ocn_split_bf16x3, ocn_label_ranks (no signature changed).
 *   109            BREAKING: one entry point per attention / token-embedding op.  ocn_attn_fwd / ocn_attn_bwd take head_dim and a nullable seq_off, order and
 *                  bucket_counts (ocn_attn_bwd also delta_ws); ocn_token_embed_fwd takes a nullable posidx, ocn_token_embed_bwd is the sorted form with a
 *                  nullable seq_off.  Gone: ocn_attn_{fwd,bwd}_hd, ocn_attn_{fwd,bwd}_varlen, ocn_token_embed_fwd_rows, ocn_token_embed_bwd_sorted[_varlen]
 *                  and the unsorted per-occurrence-atomic ocn_token_embed_bwd.
 *   110            Muon optimizer: new ocn_gemm_nt_batched, ocn_muon_momentum_multi, ocn_muon_normalize_multi, ocn_muon_apply_multi, ocn_muon_axpby
 *                  (no signature changed).
 *   111            NAdamW optimizer: new ocn_nadamw_multi (no signature changed).
 *   112            RandomResizedCrop on the device: new ocn_resized_crop_u8 (no signature changed).
 *   113            colour jitter and grayscale on the device: new ocn_color_jitter_u8 (no signature changed).
 *   114            ragged sources and the validation transform on the device: new ocn_resample_u8 (no signature changed).
 *   115            model EMA: new ocn_ema_lerp_multi (no signature changed).
 *   116            distillation: new ocn_distill_rows (no signature changed).
 *   116 (still)    position tables at another image size / context length: new ocn_pos_resample_fwd, ocn_pos_resample_bwd.  No signature changed, and
 *                  the number stays: tests/test_distill.py pins 116, and a library built before the two entry points existed fails at load on the
 *                  missing symbols, not later. */
#define OCN_ABI_VERSION 116
int ocn_version(void);

/* ---- GEMMs (MFMA v_mfma_f32_32x32x16_bf16, fp32 accumulate) ------------------------------------
 * ocn_gemm_nt: C[M,N] = A[M,K] . B[N,K]^T with a fused epilogue.  Replaces F.linear
 *   (transformer.py:169 in_proj, :246 out_proj, :295-299 c_fc + nn.GELU + c_proj), the residual adds of
 *   transformer.py:328-329, `pooled @ proj` (:923), `x @ text_projection` (model.py:409), the logit
 *   matmul (loss.py:103-110) and every dgrad of the backward (a17).  K % 32 == 0; A, B bf16 row-major.
 *   bias [N] fp32 or NULL; resid fp32 [M,ldc] (EPI 2) or bf16 [M,ldc] (EPI 8); aux uint8 [M,ldc] (EPI 1: written, EPI 3: read): the GELU derivative, the only
 *   thing the backward needs of the pre-activation, as q = round((gelu' + 0.13) * 200) in [0, 252] -- gelu' lies in [-0.129, 1.129], so
 *   the decoded value q / 200 - 0.13 is within 0.0025 of it (unbiased; rms 0.0014, what rounding a value in [0.5, 1) to bf16 costs) at
 *   half the bytes of a bf16 copy.  Alignment: lda, ldb % 8 == 0; A, B, out, bias and resid on 16 bytes, aux on 8 (checked; operands may be
 *   views of larger matrices: a row stride and a base pointer are all the kernels take). */
int ocn_gemm_nt(int epilogue, const void* A, int lda, const void* B, int ldb, void* out, int ldc, int M, int N, int K,
                const float* bias, const void* resid, void* aux, float alpha, ocn_stream_t stream);

/* ocn_gemm_tn_accum: dW[N,K] += alpha * A[M,N]^T . B[M,K]  (fp32 atomics into dW, which the caller zeroes or
 *   pre-loads); if dbias != NULL also dbias[N] += alpha * colsum(A).  The wgrad + bias-grad of every Linear
 *   (autograd of transformer.py:169,246,295-299) and the G^T products of the loss backward.
 *   N % 8 == 0, K % 8 == 0; M arbitrary. */
int ocn_gemm_tn_accum(const void* A, int lda, const void* B, int ldb, float* dW, int ldw, int M, int N, int K,
                      float* dbias, float alpha, ocn_stream_t stream);

/* Two weight gradients over the SAME M rows and the same K in ONE launch (both bias gradients or neither):
 *   dW1[N1,K] += alpha * A1[M,N1]^T . B1[M,K],  dW2[N2,K] += alpha * A2[M,N2]^T . B2[M,K].
 * The out-proj and QKV weight gradients of a residual block (autograd of transformer.py:169,246) are such a pair: alone, the small one
 * needs 28-64 M-splits to fill the chip and spends 26-37 % of its time in contended atomics; paired they share 7 splits.  Shapes the
 * paired kernel does not take are executed as two ocn_gemm_tn_accum calls (same results up to fp32 summation order). */
int ocn_gemm_tn_accum2(const void* A1, int lda1, const void* B1, int ldb1, float* dW1, int ldw1, float* dbias1, int N1,
                       const void* A2, int lda2, const void* B2, int ldb2, float* dW2, int ldw2, float* dbias2, int N2,
                       int M, int K, float alpha, ocn_stream_t stream);

/* Split-K form of ocn_gemm_nt for products with FEW output tiles and a LONG K (the loss's `G @ T` of loss.py:103-110's backward: [4096, 512] from
 * K = 32768 has 32 tiles for 256 CUs): K is cut into `ksplit` slices, every slice of every 256 x 256 tile is a tile of the persistent kernel's walk and
 * leaves its fp32 partial sum in slab s of `workspace` (ksplit * M * ldc floats); a second kernel forms
 *   out[m, n] = scale * (rowscale[m] * sum_s ws[s][m][n] - sub_alpha * sub_rows[m][n])
 * (rowscale fp32 [M], sub_rows bf16 [M, ld_sub], scale_dev a 1-element DEVICE value: each may be NULL) -- the row scale of the one-pass cross-entropy,
 * the exact -onehot part of the logit gradient and logit_scale, which the caller would otherwise apply in four more passes over out.
 * ocn_gemm_nt_splitk_plan: the ksplit that fills the chip (1 = no split: use ocn_gemm_nt).  K % (128 * ksplit) == 0. */
int ocn_gemm_nt_splitk_plan(int M, int N, int K);
int ocn_gemm_nt_splitk(const void* A, int lda, const void* B, int ldb, float* out, int ldc, int M, int N, int K, int ksplit, float* workspace,
                       const float* rowscale, const void* sub_rows_bf16, int ld_sub, float sub_alpha, const float* scale_dev, ocn_stream_t stream);

/* Run-to-run reproducible form of ocn_gemm_tn_accum (same arguments, same result up to fp32 summation ORDER, which here is fixed): no
 * two workgroups add into one address.  Shapes the hand-scheduled kernel takes (ocn_gemm_tn_det_workspace_bytes(M, N, K) > 0) need that
 * many bytes of 16-byte aligned scratch: every M-split stores its partial dW tile (and bias row) to its own slab and a second kernel sums
 * the slabs in split order; other shapes run the general kernel with one M-split and need no scratch.  The reference's counterpart is
 * torch.use_deterministic_algorithms for its own GEMMs; cost here: one extra pass over splits x N x K floats per launch. */
int64_t ocn_gemm_tn_det_workspace_bytes(int M, int N, int K);
int ocn_gemm_tn_accum_det(const void* A, int lda, const void* B, int ldb, float* dW, int ldw, int M, int N, int K, float* dbias,
                          float alpha, void* workspace, int64_t workspace_bytes, ocn_stream_t stream);

/* ---- casts -------------------------------------------------------------------------------------
 * amp_bf16 policy (precision.py:6-16): fp32 master weights, bf16 GEMM operands. */
int ocn_cast_f32_bf16(const float* src, void* dst, int64_t n, ocn_stream_t stream);
/* the widening twin, dst fp32 = src bf16 (exact).  An image tower built with `no_ln_pre` (nn.Identity at transformer.py:660) has no LayerNorm backward
 * in front of its embedding that would hand the bf16 stream's gradient on in fp32: this cast does, once per step (autograd of transformer.py:794-808
 * under autocast, where the gradient of conv1's bf16 output is widened by the cast's own backward).  src, dst 16-byte aligned; any n > 0. */
int ocn_cast_bf16_f32(const void* src, float* dst, int64_t n, ocn_stream_t stream);
/* dst = bf16(src * *scale_dev): the scalar is read on the device, so a caller that holds it in a tensor (logit_scale.exp(),
 * loss.py:103-110) never has to synchronise the host to pass it */
int ocn_cast_f32_bf16_scaled(const float* src, void* dst, int64_t n, const float* scale_dev, ocn_stream_t stream);
/* dst[C,R] (bf16) = transpose(src[R,C] fp32): weight copies laid out for the NT dgrad / `@ proj` GEMMs */
int ocn_cast_transpose_f32_bf16(const float* src, void* dst, int R, int C, ocn_stream_t stream);

/* ---- LayerNorm (layers.py:20-26, eps 1e-5; fp32 statistics) ------------------------------------
 * fwd: y = (x-mean)*rstd*w + b over the last dim C (C % 4 == 0, C <= 2048); writes y as bf16 and/or fp32
 *      (either pointer may be NULL) and mean/rstd [M] for the backward.
 * bwd: dx = LN'(dy) (+ dres if non-NULL: the residual branch's gradient), written as fp32 and/or bf16;
 *      dw[C] += sum_rows dy*xhat, db[C] += sum_rows dy (fp32 atomics; caller zeroes).
 *      dy is bf16 (dy_is_f32 = 0) or fp32 (1).
 *      dcol (may be NULL): dcol[C] += sum_rows dx in fp32, before dx is rounded to bf16.  dx is the gradient of the output of the linear
 *      in front of this LayerNorm's input (out_proj, or the previous block's c_proj: transformer.py:246, :299), so this is that layer's bias
 *      gradient summed from fp32 values instead of from the bf16 operand of its weight-gradient GEMM.
 * ocn_colsum_f32: out[C] += sum_rows x[R, C] (fp32; the same for tensors no LayerNorm backward produces).
 * bf16 residual stream (round 6; the IMAGE tower as the reference's autocast runs it: transformer.py:794 conv1 under autocast -> bf16,
 *      layers.py:23-26 `x.to(orig_type)`): x is fp32 (x_is_bf16 = 0) or bf16 (1); in the backward a bf16 x takes a bf16 dy, no dcol, and the
 *      residual gradient dres as bf16 (dres_is_bf16 = 1: the gradient of a bf16 tensor is bf16 under autograd) or fp32.  Statistics and
 *      arithmetic are fp32 in every form. */
int ocn_layernorm_fwd(const void* x, int x_is_bf16, const float* w, const float* b, void* y_bf16, float* y_f32, float* mean,
                      float* rstd, int M, int C, float eps, ocn_stream_t stream);
int ocn_layernorm_bwd(const void* dy, int dy_is_f32, const void* x, int x_is_bf16, const float* w, const float* mean,
                      const float* rstd, const void* dres, int dres_is_bf16, float* dx_f32, void* dx_bf16, float* dw, float* db, float* dcol,
                      float* det_workspace, int M, int C, ocn_stream_t stream);
/* det_workspace (may be NULL = fp32 atomics): ocn_layernorm_bwd_det_workspace_floats(M, C) floats; the workgroups' partial dw / db / dcol rows go to
 * their own slabs and a second kernel adds them in workgroup order: bit-reproducible from run to run (torch.use_deterministic_algorithms) */
int64_t ocn_layernorm_bwd_det_workspace_floats(int M, int C);
int ocn_colsum_f32(const float* x, float* out, int R, int C, int deterministic, ocn_stream_t stream);
/* ---- attention core (transformer.py:199-244: head split + F.scaled_dot_product_attention) ------
 * qkv bf16 [rows, 3*H*head_dim] (q | k | v column blocks, heads contiguous inside each: the layout F.linear with in_proj_weight produces,
 * transformer.py:169); out bf16 [rows, H*head_dim]; lse fp32 [B*H*L] (natural log).  causal != 0 applies the text tower's upper-triangular
 * -inf mask (transformer.py:1716-1722) as a predicate.
 * Layout of the rows:
 *   seq_off == NULL: a dense batch, sequence b owns rows b*L .. (b+1)*L.  order and bucket_counts must be NULL too.
 *   seq_off != NULL: a packed ("varlen") batch.  The text tower pools x[b, argmax(text[b])] (transformer.py:941-944) under the causal mask, so the
 *     tokens behind the pooled one cannot influence the feature or any gradient: the native text tower keeps only the first eot[b]+1 tokens of each
 *     sequence.  Sequence b owns rows seq_off[b] .. seq_off[b+1] (seq_off: B+1 ascending int32 on the device, 1 <= length <= L = Lmax); lse keeps the
 *     dense [B,H,L] layout.  Bucketing (optional; both pointers or neither): `order` = the B sequence ids grouped by ceil(length / 32) ascending
 *     (DEVICE, from ocn_seq_bucket_plan), `bucket_counts` = how many sequences each group holds (HOST array of ceil(L / 32) ints summing to B).  One
 *     launch per non-empty group, its workgroups sized for that group's length instead of L (these kernels are latency-bound: their rate is the
 *     number of resident workgroups); results do not depend on the bucketing.
 *   Anything else is refused before any launch.
 * Kernels: a packed batch runs the head-resident kernels of csrc/attention.hip (one workgroup per head) and needs head_dim == 64 and L <= 320, else
 *   OCN_ERR_UNSUPPORTED.  A dense batch runs them for head_dim 64 up to 128 tokens (forward) / 320 tokens (backward), and for everything else -- head_dim
 *   80, 88, 96, 104, 112 or 128 (ViT-H-14, ViT-g / bigG / e), ViT-L-14's 257 tokens -- the STREAMED kernels of csrc/attention_generic.hip: 4-wave
 *   workgroups that own four 32-row blocks and stream the operand all of them need through a two-slot LDS ring in 64-row chunks (18-35 KB of LDS per
 *   workgroup, any sequence length).  The streamed backward needs the workspace `delta_ws`, fp32 [B*H*L] (sum_d dO*O, exchanged between its launches);
 *   it may be NULL whenever the head-resident kernels are taken. */
int ocn_attn_fwd(const void* qkv, void* out, float* lse, const int32_t* seq_off, const int32_t* order, const int32_t* bucket_counts, int B, int L,
                 int H, int head_dim, int causal, float scale, ocn_stream_t stream);
int ocn_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, float* delta_ws, const int32_t* seq_off,
                 const int32_t* order, const int32_t* bucket_counts, int B, int L, int H, int head_dim, int causal, float scale, ocn_stream_t stream);

/* Single-query attention of a tower's LAST block, head_dim 64 (csrc/attention_pooled.hip).  Both poolers read one row per sequence of the
 * last block's output (transformer.py:829-831 `x[:, 0]`, :941-944 `x[arange, text.argmax(-1)]`), and rows only mix inside the attention: of
 * that block's attention exactly one query per (sequence, head) is needed.  q / out / dout / dq are [B, H*64] (the pooled rows), kv / dkv
 * [M, 2*H*64] (K | V column blocks of EVERY row: F.linear with in_proj_weight[C:], transformer.py:169), lse fp32 [B*H].  Sequence b owns rows
 * seq_off[b] .. seq_off[b+1] of kv (packed text rows) or, with seq_off = NULL, rows b*L .. (b+1)*L; rows[b] = absolute row of its pooled
 * token, which under `causal` sees the keys up to and including its own row.  The backward writes every key row of dkv (zeros behind the
 * pooled row). */
int ocn_attn_pooled_fwd(const void* q, const void* kv, void* out, float* lse, const int32_t* seq_off, const int32_t* rows, int B, int L,
                        int H, int causal, float scale, ocn_stream_t stream);
int ocn_attn_pooled_bwd(const void* q, const void* kv, const void* out, const void* dout, const float* lse, void* dq, void* dkv,
                        const int32_t* seq_off, const int32_t* rows, int B, int L, int H, int causal, float scale, ocn_stream_t stream);

/* ---- patch dropout: which patches survive (transformer.py:17-58 PatchDropout; built at :658, applied at :804 behind class token and positions) ----
 * The reference embeds all G patches and then gathers K = max(1, int(G * (1 - prob))) random ones per image (:47-56).  Which ones survive does
 * not depend on their values: here they are chosen first and only those K are patchified, multiplied and assembled (`keep` / `inv` below).
 * ocn_patch_keep_plan (transformer.py:47-51, the keep count, `randn(batch, num_tokens)` + `topk(num_patches_keep)`): for every image a 32-bit key per patch
 *   from Philox4x32-10 with counter (g, b, 0, 0) and key `seed` -- a function of (seed, b, g) alone -- and the K largest keys kept (ties by index):
 *   a uniformly random K-subset.  keep int32 [B, K]: the kept patch indices of image b ASCENDING; inv int32 [B, G]: position of patch g in
 *   keep[b], or -1.  Nothing comes back to the host.  1 <= K <= G <= 4096; one workgroup per image.
 * ocn_patch_keep_inverse (the index map autograd keeps for the gather of transformer.py:53): inv of a keep the CALLER supplies (any order; the K indices
 *   of an image must be distinct and inside [0, G) -- an index outside is clamped by every kernel that reads keep, so no access leaves a buffer). */
int ocn_patch_keep_plan(int64_t seed, int B, int G, int K, int32_t* keep, int32_t* inv, ocn_stream_t stream);
int ocn_patch_keep_inverse(const int32_t* keep, int32_t* inv, int B, int G, int K, ocn_stream_t stream);

/* ---- device-side resampling: the train crop and the validation transform in one form ----------------------------------------------------
 * (transform.py:435-440 RandomResizedCrop(image_size, scale, interpolation=BICUBIC); :461-492 image_transform(is_train=False): Resize /
 * ResizeKeepRatio + CenterCrop / CenterCropOrPad).  One tile routine (csrc/resample.hip) behind two entry points.
 * ocn_resample_u8: RAGGED sources.  arena uint8 [arena_bytes], one device buffer (base 16-byte aligned, arena_bytes a positive multiple of 4);
 *   offsets int64 [B] ON THE DEVICE = the byte offset of image b in the arena, a multiple of 16; image b is HWC uint8, tightly packed, Hs * Ws * 3
 *   bytes; plan int32 [B, 10] ON THE DEVICE = (Hs, Ws, top, left, nh, nw, Rh, Rw, oy, ox); out uint8 [B, Ho, Wo, 3]; fill in [0, 255], written to all
 *   three channels.
 *   Per axis (y shown, x alike): output row o is row r = o + oy of the image virtually resized to Rh rows; r < 0 or r >= Rh: the pixel is fill.
 *   Otherwise scale = nh / Rh, support = 2 max(scale, 1), center = scale (r + 0.5), taps k in [max(0, int(center - support + 0.5)),
 *   min(nh, int(center + support + 0.5))) with weight cubic((k - center + 0.5) / max(scale, 1)) (Keys' cubic, a = -0.5) divided by their sum; tap k
 *   reads source row top + k: the filter sees the window [top, top + nh) x [left, left + nw) and nothing else.
 *   out = round(clamp(sum_y sum_x wy wx pixel, 0, 255)), summed in fp32, ties to even.  The train crop is the plan
 *   (Hs, Ws, top, left, h, w, Ho, Wo, 0, 0), the validation transform (Hs, Ws, 0, 0, Hs, Ws, Rh, Rw, oy, ox).  With the whole image as the window
 *   this is torch's F.interpolate(image.float(), (Rh, Rw), mode="bicubic", antialias=True, align_corners=False), windowed, clamped and rounded ONCE.
 *   It is NOT PIL-compatible: PIL rounds (and clips) an 8-bit intermediate between its two passes, and on whole-image resizes the two differ by
 *   many levels where the cubic overshoots.
 *   Refused before any launch: B < 1, Ho or Wo outside [1, 1024], fill outside [0, 255], a null or misaligned operand, arena_bytes not a positive
 *   multiple of 4.  offsets and plan are never read back, so the kernel makes any content harmless:
 *     Hs, Ws are forced into [1, 8192], Rh, Rw into [1, 4096], nh into [1, min(4 Rh, 8192)] and nw alike (window anchored at its top-left corner; at
 *     most 17 taps per axis), top, left into [-32768, 32768], oy, ox into [-4096, 4096];
 *     every source coordinate is forced into [0, Hs) x [0, Ws) (a window that reaches outside sees the edge pixel repeated);
 *     the offset is forced into [0, arena_bytes - 4] and down to a multiple of 4, and the address of every byte then read, offset + (y Ws + x) 3 + c,
 *     into [0, arena_bytes) (an image that runs past the arena's end reads the arena's last byte there).
 *   Nothing is read outside the arena or written outside out, whatever the two tensors hold.  The host-side builders and check
 *   (input_pipeline.eval_resample_plan / train_resample_plan / pack_images / check_resample_plan) produce none of these forms.
 * ocn_resized_crop_u8: sources of ONE size.  src uint8 [B, Hs, Ws, 3] (HWC, what ocn_patchify_u8(hwc = 1) reads; any byte alignment), boxes int32
 *   [B, 4] = (top, left, height, width) ON THE DEVICE, out uint8 [B, Ho, Wo, 3]: the arithmetic above on the plan
 *   (Hs, Ws, top, left, height, width, Ho, Wo, 0, 0) of every image -- crop, then antialiased bicubic resize, rounded once; the taps are clamped to the
 *   crop, not to the source, and no pixel is fill: F.interpolate(crop.float(), (Ho, Wo), mode="bicubic", antialias=True, align_corners=False), clamped
 *   and rounded.  It is NOT bit-compatible with PIL's fixed-point resampler (8-bit intermediate): the two differ by at most one level on roughly a
 *   sixth of noise values.
 *   1 <= Ho, Wo <= 1024 and 1 <= Hs, Ws <= 8192, refused before any launch.  The boxes are never read back, so the kernel makes a bad one harmless:
 *   a side is forced into [1, 4 * output side] (box anchored at its top-left corner; at most 17 taps per axis) and every source coordinate into the
 *   image (a box that reaches outside reads the edge pixel repeated) -- no access leaves src whatever boxes holds.  The host-side builders
 *   (input_pipeline.random_resized_crop_boxes / check_boxes) never produce either form. */
int ocn_resized_crop_u8(const void* src_u8, int B, int Hs, int Ws, const int32_t* boxes, void* out_u8, int Ho, int Wo, ocn_stream_t stream);
int ocn_resample_u8(const void* arena_u8, int64_t arena_bytes, const int64_t* offsets, const int32_t* plan, int B, void* out_u8, int Ho, int Wo, int fill,
                    ocn_stream_t stream);

/* ---- position tables at another size (model.py:790-854 resize_pos_embed / resize_text_pos_embed; csrc/pos_resample.hip) -------------------
 * ocn_pos_resample_fwd: src fp32 [prefix + Hs*Ws, C] -> dst fp32 [prefix + Ho*Wo, C], both row-major, channels last as the parameter is stored.  The
 *   `prefix` rows (the class token: 1, or 0) are copied; the grid rows are F.interpolate(grid [1, C, Hs, Ws], size=(Ho, Wo), mode, antialias,
 *   align_corners=False) per channel, mode 0 = (bi)linear, 1 = bicubic.  The 1-D text table is Hs = Ho = 1.  Per axis, length n -> R, c2 = n (2r + 1):
 *     antialias = 1:  M = max(n, R), K = 2 (cubic) / 1 (linear); taps k in [max(0, (c2 - 2KM + R) / 2R), min(n, (c2 + 2KM + R) / 2R)), weight
 *                     f(((2k + 1) R - c2) / 2M) / (the window's sum, added in tap order); f = Keys' cubic with a = -0.5, or max(0, 1 - |x|)
 *     cubic:          x = (c2 - R) / 2R, f0 = floor(x), t = x - f0: taps f0 - 1 .. f0 + 2, each index clamped to [0, n - 1] (clamped taps add up on the
 *                     border element), weights cubic(j - 1 - t) with a = -0.75, not renormalised
 *     linear:         x = max((c2 - R) / 2R, 0), f0 = min(int(x), n - 1), t = x - f0: 1 - t on f0, t on min(f0 + 1, n - 1)
 *   Tap positions come from exact integers; the one division per weight argument is their only rounding.  Taps of weight exactly 0 are dropped, so an
 *   axis whose two lengths are equal is the identity: the result holds the source's bits.  Summation, fp32 with fused multiply-adds, in ONE order:
 *   dst = sum_y wy * (sum_x wx * src), the inner sum first, taps in increasing order, each sum started with its first product: the same bits every run.
 * ocn_pos_resample_bwd: the transposed map dsrc = W^T ddst (ddst fp32 [prefix + Ho*Wo, C] -> dsrc fp32 [prefix + Hs*Ws, C], every row written, prefix
 *   rows copied) in gather form: every source element sums, over the outputs whose taps hold it in increasing output index (rows outside, columns
 *   inside), the weight the forward gives it there.  No atomic: the same bits every run.
 * Lanes run along C: float4 where C % 4 == 0 and both tables are 16-byte aligned, scalar otherwise; any C >= 1.
 * Refused before any launch, the argument named: a grid side outside [1, 64]; a 1-D linear call (Hs = Ho = 1, mode 0) with a length outside [1, 4096]
 *   (forward; the backward takes sides up to 64 only) or with antialias = 1 (torch raises there too); mode or antialias outside {0, 1}; prefix outside
 *   [0, 64]; C < 1; a null or misaligned table. */
int ocn_pos_resample_fwd(const float* src, float* dst, int prefix, int Hs, int Ws, int Ho, int Wo, int C, int mode /*0 linear, 1 cubic*/, int antialias,
                         ocn_stream_t stream);
int ocn_pos_resample_bwd(const float* ddst, float* dsrc, int prefix, int Hs, int Ws, int Ho, int Wo, int C, int mode, int antialias,
                         ocn_stream_t stream);

/* ---- device-side colour jitter and grayscale (transform.py:335-364, :442-450: color_jitter(*aug_cfg.color_jitter, p), gray_scale(p)) ----------
 * ocn_color_jitter_u8: img uint8 [B, H, W, 3] (HWC), factors fp32 [B, 4] = (brightness, contrast, saturation, hue) and plan int32 [B] ON THE DEVICE,
 *   mean_ws fp32 [B] (workspace: the contrast means), out uint8 [B, H, W, 3]; out == img (in place) is allowed, any other overlap is not.
 *   plan[b]: bits 0-11 = four 3-bit step codes executed from the low bits up (0 nothing, 1 brightness, 2 contrast, 3 saturation, 4 hue; 5-7 are
 *   treated as nothing), bit 12 = grayscale behind the steps.  A code of 0 is how "this step is absent" is written (torchvision drops a step whose
 *   range is degenerate); a jitter that was not applied is four zeros.  factors[b] is read by code, whatever the order of the steps.
 *   THE ARITHMETIC (ours: torchvision's tensor path on a float image -- F.adjust_brightness / contrast / saturation / hue, F.rgb_to_grayscale -- with
 *   ONE rounding at the end; no bit-compatibility with torchvision's uint8 path or PIL's ImageEnhance is claimed: those quantise to 8 bits after
 *   every step, PIL rounds the grayscale weights to 16-bit integers and turns the hue of an 8-bit HSV image).  Per image, in fp32, x = u8 / 255 per
 *   channel, gray(x) = 0.2989 r + 0.587 g + 0.114 b; every step ends in clamp(., 0, 1):
 *     brightness f: x <- f x.
 *     contrast f:   x <- f x + (1 - f) m, m = the mean of gray(x) over all pixels of the image as it stands when the (first) contrast step is
 *                   reached: the steps in front of it applied, their clamps included.  The kernel sums gray rounded to multiples of 2^-24 in
 *                   integers (m is within 2^-25 of the mean of the fp32 grays): the sum does not depend on the order of its terms, so m does not
 *                   depend on the launch or on the alignment of the image.  No float atomics.
 *     saturation f: x <- f x + (1 - f) gray(x), per pixel.
 *     hue h in [-0.5, 0.5]: rgb -> hsv, hh <- (hh + h) mod 1 in [0, 1), hsv -> rgb, with
 *       rgb -> hsv: maxc, minc, cr = maxc - minc, eq = (maxc == minc); s = cr / (eq ? 1 : maxc); (rc, gc, bc) = (maxc - (r, g, b)) / (eq ? 1 : cr);
 *                   hh = [maxc == r] (bc - gc) + [maxc == g and maxc != r] (2 + rc - bc) + [maxc != g and maxc != r] (4 + gc - rc);
 *                   hh <- fmod(hh / 6 + 1, 1); v = maxc;
 *       hsv -> rgb: i = floor(6 hh), f = 6 hh - i, i <- i mod 6; p = clamp(v (1 - s)), q = clamp(v (1 - s f)), t = clamp(v (1 - s (1 - f)));
 *                   (r, g, b) = (v,t,p) (q,v,p) (p,v,t) (p,q,v) (t,p,v) (v,p,q) for i = 0..5.
 *     grayscale (bit 12): r = g = b <- gray(x).
 *     out = round-half-even(255 x), the one rounding (torchvision truncates 255.999 x; this rounds, as the crop does).
 *   The kernel multiplies by the rounded reciprocals of 255 and 6 and takes 1 / maxc and 1 / cr from v_rcp_f32 (1 ulp); results are judged against a
 *   float64 evaluation of the above with a band of 2^-9 levels around .5 (tests/color_jitter_util.py).
 *   An image whose plan holds no step and no grayscale comes out BIT-IDENTICAL: it is copied, not run through identity factors (the hue round
 *   trip is not exact in fp32 even at h = 0); in place it is not touched at all.
 *   Two launches: the contrast means (one workgroup per image with a contrast step), then the chain per pixel; a thread owns 4 consecutive pixels =
 *   12 bytes = three dwords where the image's address allows, single pixels by bytes in front of and behind them, the same arithmetic either way.
 *   1 <= H, W <= 8192, refused before any launch.  NO ADDRESS DEPENDS ON factors OR plan: whatever they hold, exactly B * H * W * 3 bytes are read and
 *   written; non-finite factors give unspecified pixel values and nothing else.  The host-side builders (input_pipeline.color_jitter_plan /
 *   check_jitter) produce neither a code above 4, a step twice, nor a non-finite factor. */
int ocn_color_jitter_u8(const void* img_u8, int B, int H, int W, const float* factors, const int32_t* plan, float* mean_ws, void* out_u8,
                        ocn_stream_t stream);

/* ---- image tower embedding (transformer.py:793-808) -------------------------------------------
 * All four take the patches of a patch-dropout step as an optional index map, G = gh*gw = (H/P)*(W/P) patches per image of which K are embedded:
 *   keep int32 [B, K] (1 <= K <= G, honoured in the order given; ocn_patch_keep_plan or the caller's) for the forward functions, its inverse inv
 *   int32 [B, G] for the backward.  keep == NULL / inv == NULL: every patch in grid order, i.e. keep[b, j] = j and inv[b, g] = g, and then K MUST
 *   equal G -- anything else is refused before any launch.
 * ocn_patchify (transformer.py:794-796): image [B,3,H,W] (fp32, or bf16 when image_is_bf16) -> patches bf16 [B*K, Kpad]; row b*K + j is patch
 *   keep[b, j] of image b, column order (c, i, j) = conv1.weight.reshape(width, 3*P*P) (:632-638); zero-padded to Kpad.  Dropped patches are never read.
 * ocn_patchify_u8, the uint8 input path (8f-4): pixels as decoded ([B,H,W,3] when hwc, else [B,3,H,W]); the kernel applies ToTensor + Normalize
 *   ((x/255 - mean[c]) / std[c]; mean3 / std3 = HOST pointers to 3 floats, src/open_clip/constants.py:1-2) while building the same bf16 patch matrix.
 * ocn_embed_assemble_fwd (:799-804; :53-56 the gather and the class token in front): emb fp32 [B, K+1, C]; emb[b,0] = cls + pos[0];
 *   emb[b,1+j] = patch_out[b*K+j] + pos[1 + keep[b,j]] -- the position is added before the drop, so a kept patch carries its own.
 * ocn_embed_assemble_bwd (autograd of the same): dpatch bf16 [B*K, C] = demb[b,1+j]; dcls[C] += sum_b demb[b,0]; dpos[0] += the same;
 *   dpos[1+g] += sum over the images with inv[b,g] >= 0 of demb[b, 1 + inv[b,g]] -- a gather per (position, channel), fp32 atomics per batch chunk
 *   or (deterministic) a single writer in batch order.  dpatch is reached through inv alone: a row of keep that inv does not point back to (a
 *   caller's keep with a repeated or clamped index) is not written -- the caller zero-fills dpatch for such a keep. */
int ocn_patchify(const void* image, int image_is_bf16, const int32_t* keep, int K, void* patches, int B, int H, int W, int P, int Kpad,
                 ocn_stream_t stream);
int ocn_patchify_u8(const void* image_u8, int hwc, const float* mean3, const float* std3, const int32_t* keep, int K, void* patches, int B,
                    int H, int W, int P, int Kpad, ocn_stream_t stream);
int ocn_embed_assemble_fwd(const float* patch_out, const float* cls, const float* pos, const int32_t* keep, float* emb, int B, int G, int K,
                           int C, ocn_stream_t stream);
int ocn_embed_assemble_bwd(const float* demb, const int32_t* inv, void* dpatch_bf16, float* dpos, float* dcls, int B, int G, int K, int C,
                           int deterministic, ocn_stream_t stream);

/* ---- text tower embedding (model.py:399-401) ---------------------------------------------------
 * Rows are the M = B*L tokens of a dense batch (row b*L + l carries position l) or the M rows of a packed one (see ocn_attn_fwd, ocn_seq_pack_rows).
 * fwd: x[r,:] = table[tokens[r],:] + pos[position of r,:] (fp32 [M,C]; tokens int64 [M]).  posidx == NULL: dense, the position is r % L and
 *   M % L == 0 is required; otherwise it is posidx[r] (int32 [M]).
 * bwd: dtable[tokens[r],:] += dx[r,:] as a segment reduce over SORTED ids (no per-occurrence atomics): sorted_tokens = the M ids in ascending order,
 *   order[i] = the row of dx that sorted_tokens[i] came from (torch.sort on the device).  dtable must arrive ZEROED (complete runs are stored, not
 *   added).  dpos[l,:] += the sum of dx over the rows at position l: seq_off == NULL: dense, rows b*L + l and M == B*L is required; otherwise
 *   rows seq_off[b] + l of the sequences longer than l.  dx is fp32 or (dx_is_bf16) bf16 [M, C], 16-byte aligned like dtable.
 * deterministic != 0 (here and in ocn_embed_assemble_bwd): the reproducible form -- every run of equal ids is summed by ONE workgroup in sorted
 *   order (needs a STABLE sort), dpos / dcls by a single writer per element in batch order: no fp32 atomics, bit-identical from run to run
 *   (torch.use_deterministic_algorithms); long runs (SOT / EOT, the zero padding of a dense batch) serialise. */
int ocn_token_embed_fwd(const int64_t* tokens, const int32_t* posidx, const float* table, const float* pos, float* x, long M, int L, int C, int vocab,
                        ocn_stream_t stream);
int ocn_token_embed_bwd(const int64_t* sorted_tokens, const int64_t* order, const void* dx, int dx_is_bf16, float* dtable, float* dpos,
                        const int32_t* seq_off, int B, int L, long M, int C, int vocab, int deterministic, ocn_stream_t stream);

/* ---- packed text batches (see ocn_attn_fwd) ------------------------------------------------------
 * seq_pack_plan: eot[b] = argmax(text[b,:]); seq_off = exclusive scan of (eot+1) (B+1 entries, seq_off[B] = packed row count M);
 *   last_row[b] = seq_off[b+1]-1 (the pooled row).  seq_pack_rows: tokens[seq_off[b]+l] = text[b,l], posidx[..] = l for l <= eot[b]. */
int ocn_seq_pack_plan(const int64_t* text, int32_t* eot, int32_t* seq_off, int32_t* last_row, int B, int L, ocn_stream_t stream);
/* *bad_count = number of ids outside [0, vocab) among text[0..n) (one workgroup, no atomics; written, not accumulated).  The embedding
 * kernels clamp such ids; nn.Embedding (src/open_clip/model.py:399) raises on them -- the host raises from this count. */
int ocn_token_range_check(const int64_t* text, long n, int vocab, int32_t* bad_count, ocn_stream_t stream);
/* order[0..B) = sequence ids grouped by ceil(length / 32) ascending, counts[k] = number of sequences with ceil(length / 32) == k + 1
 * (ceil(Lmax / 32) <= 16 entries, device): the buckets of ocn_attn_fwd / ocn_attn_bwd.  The order inside a bucket is unspecified. */
int ocn_seq_bucket_plan(const int32_t* seq_off, int32_t* order, int32_t* counts, int B, int Lmax, ocn_stream_t stream);
int ocn_seq_pack_rows(const int64_t* text, const int32_t* seq_off, int64_t* tokens, int32_t* posidx, int B, int L, ocn_stream_t stream);

/* ---- pooling (transformer.py:786-787 'tok'; :941-944 'argmax') ---------------------------------
 * argmax_rows: idx[b] = first index of max(text[b,:]) (torch.argmax semantics)
 * gather_rows: out[b,:] = x[(b*L + idx[b]),:] (idx NULL -> token 0);  scatter_rows: dx (pre-zeroed)[b*L+idx[b],:] = d[b,:]
 *   (L = 0: idx holds absolute row numbers -- the packed text tower's last_row) */
int ocn_argmax_rows(const int64_t* text, int32_t* idx, int B, int L, ocn_stream_t stream);
int ocn_gather_rows(const void* x, int x_is_bf16, const int32_t* idx, float* out, int B, int L, int C, ocn_stream_t stream); /* x fp32 or bf16; out fp32 */
int ocn_gather_rows_bf16(const void* x, const int32_t* idx, void* out, int B, int L, int C, ocn_stream_t stream); /* bf16 x / out, C % 8 == 0 */
int ocn_scatter_rows(const float* d, const int32_t* idx, float* dx, void* dx_bf16, int B, int L, int C,
                     ocn_stream_t stream);
/* dx[row_b] += d[b] (fp32), dx_bf16[row_b] = bf16 of the sum (may be NULL): the pooled rows' share of the last block's input gradient added
 * into the all-row LayerNorm backward's result instead of travelling through a zero [M, C] residual-gradient matrix.  dx = NULL (bf16
 * gradient stream): dx_bf16[row_b] = bf16(dx_bf16[row_b] + d[b]). */
int ocn_scatter_add_rows(const float* d, const int32_t* idx, float* dx, void* dx_bf16, int B, int L, int C, ocn_stream_t stream);

/* ---- mean pooling ('avg': `x[:, 1:].mean(dim=1)`, transformer.py:783-785; the CLIPA image towers) ----------------------------
 * fwd: out[b, c] = (sum_{t = skip .. T-1} x[b*T + t, c]) / float(T - skip); x [B*T, C] fp32 or bf16 (x_is_bf16), out fp32 [B, C].  fp32 accumulation in
 *      one fixed order (the tokens of an image dealt out over the waves of a workgroup, the partial sums added in wave order), then ONE correctly
 *      rounded fp32 division: bit-reproducible, and exact whenever the sum is.  Rows t < skip are never read.
 * bwd: autograd of the same line: every row of [B*T, C] is written -- rows t < skip exact zeros, the others dpooled[b, c] / float(T - skip) -- as fp32
 *      (dx), as its round-to-nearest-even bf16 (dx_bf16), or both in one pass; either pointer may be NULL, not both.  Nothing has to be zeroed first.
 * Checked on the host before any launch: no null operand, B, C > 0, 0 <= skip < T, C % 8 == 0, 16-byte aligned operands. */
int ocn_mean_pool_fwd(const void* x, int x_is_bf16, float* out, int B, int T, int skip, int C, ocn_stream_t stream);
int ocn_mean_pool_bwd(const float* dpooled, float* dx, void* dx_bf16, int B, int T, int skip, int C, ocn_stream_t stream);

/* ---- F.normalize (model.py:391,411; eps 1e-12) -------------------------------------------------
 * fwd: y = x / max(||x||, eps) as fp32 and bf16, inv_norm[B] saved; bwd: dx = (dy - y*(y.dy)) * inv_norm */
int ocn_l2norm_fwd(const float* x, float* y, void* y_bf16, float* inv_norm, int B, int E, float eps, ocn_stream_t stream);
int ocn_l2norm_bwd(const float* dy, const float* y, const float* inv_norm, float* dx, int B, int E, ocn_stream_t stream);

/* ---- contrastive losses on materialised logits -------------------------------------------------
 * softmax CE rows (F.cross_entropy(logits, arange+offset), loss.py:78-89,136-139): for each of R rows of
 *   logits fp32 [R,N]: lse, loss_sum += (lse - logits[r, r+label_offset]) * loss_scale; writes
 *   G bf16 [R,N] = softmax * grad_scale -- the -onehot * grad_scale part of the logit gradient is NOT stored: the caller applies it exactly in
 *   fp32 (dX_r -= grad_scale * Y[r + label_offset], dY[r + label_offset] -= grad_scale * X_r): rounded to bf16 the label entry
 *   (p - 1) * grad_scale loses its p, a bias of the same sign in every row that every sum over the batch adds up coherently;
 *   dscale_sum += sum((softmax - onehot) * grad_scale * logits) * inv_logit_scale.
 * siglip (loss.py:344-367): z = labels*logits (labels -1 off-diagonal, +1 on (r, r+label_offset) unless
 *   negative_only); loss_sum += -logsigmoid(z)*loss_scale; with g = -labels*sigmoid(-z) = sigmoid(logits) - [positive]: G =
 *   sigmoid(logits)*grad_scale (the positives' -grad_scale is the caller's, exact, as for the cross-entropy);
 *   dscale_sum += sum(g*grad_scale*(logits-bias))*inv_logit_scale; dbias_sum += sum(g*grad_scale). */
int ocn_softmax_ce_rows(const float* logits, int ld, void* G, int ldg, int R, int N, int label_offset, float loss_scale,
                        float grad_scale, float inv_logit_scale, float* loss_sum, float* dscale_sum, float* det_rows,
                        ocn_stream_t stream);
/* det_rows (may be NULL = fp32 atomics into the three sums): fp32 [R, 3]; row r's contributions to loss_sum / dscale_sum / dbias_sum are
 * written there instead, for the caller to add up in a fixed order (ocn_colsum_f32(..., deterministic = 1)): the reproducible form */
/* distillation rows (DistillClipLoss.dist_loss, loss.py:189-190, both logit matrices materialised): for each of R rows of the student's logits
 *   l fp32 [R,N] (row stride ld_s) and the teacher's t fp32 [R,N] (row stride ld_t), p = softmax(l), q = softmax(t) -- both from ONE device routine
 *   (row maximum, sum of __expf(v - maximum), one reciprocal), so l == t gives G == 0 exactly, and nothing overflows for finite logits:
 *   loss_sum += (lse(l) - sum_j q_j l_j) * loss_scale;  G bf16 [R,N] = (p - q) * grad_scale -- the whole logit gradient: there is no label part;
 *   dscale_sum += sum_j (p_j - q_j) * grad_scale * l_j * inv_logit_scale.  det_rows as above (slot 2 = 0).  Each matrix is read twice (an online
 *   maximum / sum pass, then the pass that writes G); 16-byte loads where the strides and base addresses allow. */
int ocn_distill_rows(const float* student, int ld_s, const float* teacher, int ld_t, void* G, int ldg, int R, int N, float loss_scale,
                     float grad_scale, float inv_logit_scale, float* loss_sum, float* dscale_sum, float* det_rows, ocn_stream_t stream);
/* The same cross-entropy WITHOUT materialised logits (loss.py:103-110 + :136-139 for a [R, N] block of logits_per_image / _per_text;
 * the row-sharded global loss of 8 GPUs has R = 4096, N = 32768): X bf16 [R, E] (already times logit_scale), Y bf16 [N, E].  ONE pass of the MFMA
 * GEMM (round 6; two until round 5): its epilogue consumes the fp32 logits tile in registers and writes G' = exp(logit - c_r) as bf16 [R, ldg] with a
 * per-row shift c_r fixed before the GEMM (the row's label logit, clamped from below so that nothing can overflow), then
 *   rowscale[r] = grad_scale / sum_j G'_rj  (fp32 [R]):  the logit gradient is  G_rj = G'_rj * rowscale[r] - [j = r + label_offset] * grad_scale -- the row
 *   scale is applied by the caller where it is free (on the [R, E] result of G' @ Y, on the [R, E] operand of G'^T @ X), the onehot part exactly as above;
 *   loss_sum += sum_r (lse_r - logit[r, r + label_offset]) * loss_scale;  dscale_sum += sum((softmax - onehot) * grad_scale * logits) (divide by
 *   logit_scale for d/d logit_scale).
 * Exact for any scale: rows whose shifted sums under- / overflow (impossible for unit vectors and logit_scale <= 78, practically for <= 150) are
 * redone from the operands with their true maximum.  E % 128 == 0, N % 8 == 0; `workspace` = ocn_fused_logits_ce_workspace_floats(R, N) floats. */
int64_t ocn_fused_logits_ce_workspace_floats(int R, int N);
int ocn_fused_logits_ce(const void* X, int ldx, const void* Y, int ldy, int R, int N, int E, int label_offset, float loss_scale,
                        float grad_scale, void* G, int ldg, float* workspace, float* rowscale, float* loss_sum, float* dscale_sum, ocn_stream_t stream);
/* the caller's side of that row scale: out_bf16[r, :] = bf16(scale[r] * x_bf16[r, :]) (the [R, E] operand of G'^T @ X), and
 * out_f32[r, :] -= (alpha / scale[r]) * x_bf16[r, :] (the label rows' -onehot part of that product, from the same rounded rows).  E % 8 == 0. */
int ocn_scale_rows_bf16(const void* x_bf16, int ldx, const float* scale, void* out_bf16, int ldo, int R, int E, ocn_stream_t stream);
int ocn_sub_scaled_rows(float* out, int ldo, const void* x_bf16, int ldx, const float* scale, float alpha, int R, int E, ocn_stream_t stream);
/* bias_dev (may be NULL): the logit bias as a 1-element DEVICE value; overrides `bias` (logit_bias is a parameter: the step never reads it on the
 * host).  It is subtracted per element inside the dscale sum -- not as bias * dbias_sum afterwards, which cancels catastrophically. */
int ocn_siglip_rows(const float* logits, int ld, void* G, int ldg, int R, int N, int label_offset, int negative_only,
                    float bias, const float* bias_dev, float loss_scale, float grad_scale, float inv_logit_scale, float* loss_sum,
                    float* dscale_sum, float* dbias_sum, float* det_rows, ocn_stream_t stream);

/* ---- validation metrics (open_clip_train/metrics.py:95-169 `_paired_retrieval_ranks`; open_clip_train/zero_shot.py:15-18 `accuracy`) ----
 * ocn_label_ranks: Q bf16 [R, K] queries, C bf16 [N, K] candidates, both dense row-major (row stride K); labels int32 [R], every value in [0, N), or
 *   NULL = paired retrieval, labels[r] = r (metrics.py:148-163; needs R <= N).  With the score s[r, j] = sum_k Q[r, k] * C[j, k] (fp32 accumulation on
 *   v_mfma_f32_32x32x16_bf16; no score ever reaches memory) and the target t[r] = s[r, labels[r]]:
 *     rank[r] = #{ j in [0, N) : s[r, j] > t[r]  or  (s[r, j] == t[r] and j < labels[r]) }      (int32 [R]; the tie rule of metrics.py:156-163)
 *   Text -> image retrieval is the same call with the operands swapped; zero-shot top-k (`100 * features @ classifier` + topk, zero_shot.py:15-18,35-37)
 *   is the same call with C = classifier^T, labels = the target class: a row is correct at k when rank < k.  A positive logit scale changes no rank and
 *   is not an argument.
 *   target fp32 [R]: workspace, holds t on return.  t comes out of the same tile routine and the same K order as every other score, so bit-identical
 *   candidate rows (duplicate captions) score bit-identically and the index rule alone orders them.  Any R >= 1, N >= 1: rows past R write nothing, columns
 *   past N are never counted.  A label outside [0, N) that only the device can see is clamped into the range (no access leaves a buffer).
 *   Checked on the host before any launch: no null operand (labels excepted), R, N >= 1, K % 32 == 0, R <= N when labels == NULL, Q and C 16-byte
 *   aligned, labels / target / rank 4-byte aligned.  Enqueues a clear of rank and two kernels; results do not vary from run to run (integer adds).
 * ocn_split_bf16x3: the operands of the fp32 mode (`--val-retrieval-precision fp32`, metrics.py:14-21).  x fp32 [R, E] -> out bf16 [R, 3 * Ep], Ep = E rounded
 *   up to a multiple of 32, every segment zero-padded: hi = bf16(x), lo = bf16(x - hi); role 0 (query) writes [hi | lo | hi], role 1 (candidate) writes
 *   [hi | hi | lo], so ONE K = 3 * Ep product is hi.hi + lo.hi + hi.lo -- every term of the fp32 product but lo.lo (relative 2^-18).  The bf16 mode is
 *   ocn_cast_f32_bf16 of the features.  x 4-byte, out 16-byte aligned; R, E >= 1. */
int ocn_split_bf16x3(const float* x, void* out, int R, int E, int role, ocn_stream_t stream);
int ocn_label_ranks(const void* Q, const void* C, const int32_t* labels, float* target, int32_t* rank, int R, int N, int K, ocn_stream_t stream);

/* ---- optimizer (train.py:181-182, image_text_task.py:91-101) --------------
 * sumsq: out[0] += sum(x^2) (grad-norm for clip_grad_norm_);
 * adamw_step: torch.optim.AdamW semantics (decoupled weight decay, bias correction), optional grad scale
 *   (clip coefficient read from device pointer clip_coef or 1.0 when NULL); also refreshes the bf16 shadow
 *   copy when w_bf16 != NULL. */
int ocn_sumsq_accum(const float* x, int64_t n, float* out, ocn_stream_t stream);
int ocn_adamw_step(float* w, const float* g, float* m, float* v, void* w_bf16, int64_t n, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int step, const float* clip_coef, ocn_stream_t stream);

/* Whole-model optimizer step in one launch (8f-1): `entries` = device array of 88-byte records
 *   { float* w; const float* g; float* m; float* v; bf16* w16n; bf16* w16t; int64 numel; int32 rows, cols, mode, pad;
 *     float lr, wd, bc1 (= 1 - beta1^step), bc2_sqrt (= sqrt(1 - beta2^step)); }
 * `chunks` = device array of int32 pairs {entry, index}: 8192-element ranges (mode 0 = 16-byte vectors, 2 = scalar) or 64x64
 * tiles of a [rows, cols] weight (mode 1; rows, cols % 64 == 0).  AdamW as ocn_adamw_step; additionally rewrites the bf16
 * operand copies w16n [rows, cols] and (mode 1) w16t [cols, rows] when non-NULL.  gnorm_sq != NULL: gradients are scaled by
 * min(1, max_norm / (sqrt(*gnorm_sq) + 1e-6)) = torch.nn.utils.clip_grad_norm_ (train.py:181); ocn_sumsq_multi accumulates
 * the squared norm of every entry's gradient into out[0]. */
int ocn_adamw_multi(const void* entries, const void* chunks, int n_chunks, float beta1, float beta2, float eps,
                    const float* gnorm_sq, float max_norm, ocn_stream_t stream);
/* torch.optim.NAdam(decoupled_weight_decay=True) over the same tables, modes, operand copies and clip coefficient as ocn_adamw_multi (one kernel
 * template, another element update).  The momentum schedule is host state; the record's four floats carry, in place of lr, wd, bc1, bc2_sqrt:
 *   decay = 1 - lr * wd;  bc2 = 1 - beta2^step;  c_g = lr (1 - mu_t) / (1 - mu_product);  c_m = lr mu_next / (1 - mu_product mu_next)
 * with mu_t = beta1 (1 - 0.5 * 0.96^(step * momentum_decay)), mu_next the same at step + 1 and mu_product the running product of mu_t.  Per element:
 *   p *= decay;  m += (g - m) one_minus_beta1;  v = v beta2 + g g one_minus_beta2;  den = sqrt(v / bc2) + eps;  p -= c_g g / den + c_m m / den.
 * one_minus_beta1 / one_minus_beta2 are arguments of their own: torch forms 1 - beta in double before it rounds to fp32, and the fp32 difference
 * 1.0f - 0.98f is 1e-6 (relative) away from that, which would sit in every element of the moments.  No atomics: the update is bit-reproducible. */
int ocn_nadamw_multi(const void* entries, const void* chunks, int n_chunks, float one_minus_beta1, float beta2, float one_minus_beta2, float eps,
                     const float* gnorm_sq, float max_norm, ocn_stream_t stream);
/* chunk_ws == NULL: every chunk adds its partial sum to out[0] with an fp32 atomic (order varies from run to run).  chunk_ws = n_chunks floats:
 * the reproducible form -- every chunk stores its partial, one workgroup adds them in chunk order (clip_grad_norm_ under deterministic=True). */
int ocn_sumsq_multi(const void* entries, const void* chunks, int n_chunks, float* out, float* chunk_ws, ocn_stream_t stream);
/* Model EMA (open_clip_amd/ema.py::NativeModelEma): ema = lerp(ema, src, weight) over every tensor of a model in one launch.  `entries` = device
 * array of 32-byte records
 *   { float* ema; const float* src; int64 numel; int32 mode, pad; }
 * `chunks` = device array of int32 pairs {entry, index}: 8192-element ranges of the entry, as ocn_adamw_multi's (mode 0 = 16-byte vectors: both
 * pointers on 16 bytes; mode 2 = scalar, for a pointer off that grid; the numel % 4 tail of a mode-0 tensor is done element by element).  Per
 * element, in fp32, torch.lerp's two-branch form -- with d = src - ema:
 *   ema = weight < 0.5 ? ema + weight * d : src - d * (1 - weight)
 * so both limits are exact: weight == 1 leaves ema == src and weight == 0 leaves ema untouched, bit for bit (for finite values).  weight is
 * 1 - decay of the average; 1 - weight is formed in fp32.  8 B read + 4 B written per element; no atomics, no LDS, no host synchronisation: the
 * update is bit-reproducible.  ema and src of one entry must not overlap, nor may two entries' ema ranges.  n_chunks == 0 launches nothing; null
 * tables, n_chunks < 0 and a non-finite weight are refused before any launch. */
int ocn_ema_lerp_multi(const void* entries, const void* chunks, int n_chunks, float weight, ocn_stream_t stream);

/* ---- Muon (open_clip_amd/optim.py::NativeMuon) ---------------------------------------------------
 * ocn_gemm_nt_batched: `batch` equal-shape problems in one launch, problem i at base + i * stride (elements):
 *   C_i[M,N] = bf16(alpha * A_i[M,K] . B_i[N,K]^T + beta * R_i[M,N]),   Ct_i[N,M] = C_i^T when Ct != NULL.
 * bf16 operands, fp32 accumulation, one rounding.  One workgroup per 128 x 128 tile and problem (grid = batch * tiles).  R and Ct may be NULL; C may
 * alias R (in place), nothing else may overlap.  M, N free; K % 32 == 0; row strides of A, B, C, R and the batch strides % 8 == 0; A, B, C, R on 16 bytes. */
int ocn_gemm_nt_batched(const void* A, int lda, int64_t strideA, const void* B, int ldb, int64_t strideB, void* C, int ldc, int64_t strideC,
                        const void* R, int ldr, int64_t strideR, void* Ct, int ldct, int64_t strideCt, int M, int N, int K, int batch,
                        float alpha, float beta, ocn_stream_t stream);
/* The multi-tensor kernels of the Muon step.  `entries` = device array of 96-byte records, one per weight (a [rows, cols] fp32 matrix):
 *   { const float* g; float* buf; float* w; bf16* w16n; bf16* w16t; bf16* xn; bf16* xt; const bf16* xfin;
 *     int32 rows, cols, ldn, ldt, chunk0, nchunks; float step (= lr * scale), decay (= 1 - lr * weight_decay); }
 * `chunks` = device array of int32 pairs {entry, tile}: the 64 x 64 tiles of every weight (ragged edges allowed), tile = row-major index.
 * xn / xt: the weight-oriented and the transposed bf16 image of X in the workspace, row strides ldn >= pad32(cols), ldt >= pad32(rows), pad32(rows) resp.
 * pad32(cols) rows; xfin: the weight-oriented image of the last iterate (row stride ldn).  gnorm_sq / max_norm: as ocn_adamw_multi.
 *   momentum:  g = grad * clip; buf += (1 - momentum)(g - buf); u = nesterov ? g + momentum (buf - g) : buf; tile partials of sum u^2 into
 *              chunk_ws[chunk0 + tile]; then one workgroup per entry adds its partials in a fixed order: inv_norm[i] = 1 / (||u_i|| + 1e-7)  (no atomics)
 *   normalize: X = bf16(u * inv_norm) into xn and xt, zero in their padding
 *   apply:     w = w * decay - step * xfin; rewrites w16n [rows, cols] and w16t [cols, rows] (rows, cols % 64 == 0) when non-NULL. */
int ocn_muon_momentum_multi(const void* entries, int n_entries, const void* chunks, int n_chunks, float momentum, int nesterov,
                            const float* gnorm_sq, float max_norm, float* chunk_ws, float* inv_norm, ocn_stream_t stream);
int ocn_muon_normalize_multi(const void* entries, const void* chunks, int n_chunks, float momentum, int nesterov, const float* gnorm_sq,
                             float max_norm, const float* inv_norm, ocn_stream_t stream);
int ocn_muon_apply_multi(const void* entries, const void* chunks, int n_chunks, ocn_stream_t stream);
/* out[rows, cols] = bf16(acc + beta * R) and outT[cols, rows] (nullable), all contiguous: completes a Newton-Schulz statement whose product came out
 * of ocn_gemm_nt in fp32 (the per-matrix backend of NativeMuon) */
int ocn_muon_axpby(const float* acc, const void* R, void* out, void* outT, int rows, int cols, float beta, ocn_stream_t stream);

/* ---- collectives (loss.py:23-54 gather_features and its backward) ------------------
 * Direct RCCL calls on the caller's stream (RCCL is bound at run time from the librccl.so the process has loaded; no link-time
 * dependency).  One process per GPU.  ocn_comm_unique_id: rank 0 makes the 128-byte id, the caller distributes it (any
 * side channel); ocn_comm_init: every rank, collectively.  dtype: 0 = fp32, 1 = bf16 (ocn_comm_broadcast also 2 = raw bytes: any other tensor, exact).  Counts are ELEMENTS per rank.
 *   allgather:           recv [world * count] = concat_r send_r [count]             (the packed [B, 2E] feature exchange)
 *   reduce_scatter_sum:  recv [count] = (sum_r send_r [world * count]) [rank slice]   (backward of the gather, loss.py:23-26)
 *   allreduce_sum:       buf [count] = sum_r buf_r, in place                         (row-sharded loss scalars, gradient buckets) */
int ocn_comm_unique_id(void* id_out_128);
int ocn_comm_init(const void* id_128, int rank, int world, void** comm_out);
int ocn_comm_destroy(void* comm);
int ocn_comm_allgather(void* comm, const void* send, void* recv, int64_t count_per_rank, int dtype, ocn_stream_t stream);
int ocn_comm_reduce_scatter_sum(void* comm, const void* send, void* recv, int64_t count_per_rank, int dtype, ocn_stream_t stream);
int ocn_comm_allreduce_sum(void* comm, void* buf, int64_t count, int dtype, ocn_stream_t stream);
/* in-place MEAN over ranks (ncclAvg): the gradient all-reduce that replaces DistributedDataParallel's reducer (base_task.py:219-232) */
int ocn_comm_allreduce_avg(void* comm, void* buf, int64_t count, int dtype, ocn_stream_t stream);
/* buf [count] on every rank = rank `root`'s, in place (ncclBroadcast): the parameter broadcast at the start of training (DDP's, base_task.py:227) */
int ocn_comm_broadcast(void* comm, void* buf, int64_t count, int dtype, int root, ocn_stream_t stream);
/* what the communicator reports about itself: *count_out = ncclCommCount (ranks RCCL connected), *rank_out = ncclCommUserRank (may be NULL) */
int ocn_comm_count(void* comm, int* count_out, int* rank_out);
/* one neighbour exchange (loss.py:226-243 `neighbour_exchange`: one isend + one irecv batched): send [count] to to_rank, recv [count] from from_rank, as
 * one grouped RCCL operation on the caller's stream; dtype as above (0 fp32, 1 bf16, 2 raw bytes) */
int ocn_comm_sendrecv(void* comm, const void* send, int to_rank, void* recv, int from_rank, int64_t count, int dtype, ocn_stream_t stream);

/* ---- the persistent GEMMs next to other streams' kernels (multi-GPU) ----------------------------
 * ocn_gemm_nt / ocn_gemm_tn_accum launch one workgroup per CU with a fixed share of the tiles.  A workgroup whose CU is held by another stream's kernel
 * (RCCL's, during the gradient all-reduce) starts only when a CU frees up and then walks its whole share alone: the launch takes up to twice as long.
 * ocn_set_tile_rescue(1) (process-wide, takes effect with the next launch) selects the kernels' rescue form: the shares stay static and no atomic enters
 * the tile loop, but workgroups that finish hand out -- entry by entry, through one counter per workgroup on a per-stream board -- the shares of workgroups
 * that have not started.  Results: ocn_gemm_nt bit-identical to the static form (every tile is computed once, by whichever workgroup), ocn_gemm_tn_accum
 * sums the same products with fp32 atomics in a different order, as between any two of its runs; the reproducible wgrad (workspace form) and launches
 * recorded into a graph (stream capture) stay static.
 * Cost without contention: one atomic per workgroup at either end of a launch.  Off by default; open_clip_amd turns it on when world_size > 1. */
int ocn_set_tile_rescue(int on);
int ocn_get_tile_rescue(void);

/* ---- self-test probes (used by tests/ to pin the hardware fragment layouts this library assumes) */
int ocn_probe_mfma32(const void* a_bf16 /*[32,16]*/, const void* b_bf16 /*[32,16] (n,k)*/, float* c /*[32,32]*/,
                     ocn_stream_t stream);
int ocn_probe_tr16(const void* in_bf16 /*[16 rows][32 cols]*/, void* out_bf16 /*[64 lanes][4]*/, ocn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
