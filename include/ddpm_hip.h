/* ddpm_hip.h — C ABI of libddpm_hip.so: the MI355X (gfx950) kernels behind the ddpm-torch hot path.
 *
 * The reference (tqch/ddpm-torch) is pure Python on ATen; it has no FFI of its own.  Each entry point below
 * replaces the ATen op class the reference invokes at the cited site (paths relative to the upstream repo);
 * the binding a maintainer would add is the ctypes table in ddpm-torch_amd/ddpm_torch/_hip.py.
 *
 * Conventions
 *   - Every pointer is a DEVICE pointer owned by the caller (PyTorch's caching allocator); the library never
 *     allocates, frees or retains memory.  "stream" is a hipStream_t; all work is enqueued on it and the call
 *     returns immediately (no synchronisation, hipGraph-capturable).  Re-entrant and thread-safe.
 *   - dtype: 0 = fp32, 1 = bf16 (activations / packed weights); parameters, statistics and gradients are fp32.
 *   - Activations are NHWC: element (b, y, x, c) at  base + ((b*H + y)*W + x)*ld + c  with a caller-chosen pixel
 *     pitch ld >= C (in elements), so channel slices of a wider buffer are valid operands (zero-copy concat).
 *     Pointers and pitches must be 16-byte aligned; channel counts are multiples of 16/sizeof(dtype).
 *   - Return value: 0 OK, 1 bad shape, 2 bad dtype, 3 misaligned, 4 launch failure, 5 null pointer.
 *   - OPERAND LIMIT.  The GEMM-shaped kernels (convolutions, weight gradients, ddpm_gemm, attention) read their operands through
 *     buffer descriptors with 32-bit byte offsets.  Their launchers return 1 (bad shape), before anything is launched, when the
 *     extent of such an operand exceeds 0x7ffffff0 bytes (2 GiB - 16).  The extent of a pitched [rows][cols] operand is
 *     ((rows - 1) * ld + cols) * sizeof(dtype), of an NHWC activation (B*H*W*ld - (ld - C)) * sizeof(dtype).  Each such entry below
 *     names the operands its limit covers; outputs, residuals and fp32 side operands are addressed with 64-bit pointers and have
 *     none.  The GroupNorm entries refuse an operand of 2^31 elements or more (see there).  ddpm_add_rows, ddpm_colsum,
 *     ddpm_upsample2x_bwd and ddpm_nchw_to_nhwc index with 64-bit arithmetic: no operand limit
 *     (tests/test_large_operands_gpu.py runs them on operands of more than 2^31 elements).  ddpm_torch's UNet checks a batch against
 *     the limit before its first launch (a ValueError naming the layer; engine.max_batch(H, W)).
 */
#ifndef DDPM_HIP_H
#define DDPM_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

/* F.conv2d 3x3/1x1 (ddpm_torch/modules.py:120-123; sites models/unet.py:36,37,41,76,79,80,127,141,201), with
 * SamePad2d(3,2)+stride 2 (modules.py:153-160, unet.py:165-167), nn.Upsample(2,"nearest") (unet.py:199),
 * the per-sample time-bias add (unet.py:86) and the residual add (unet.py:60,89) fused:
 *   y[b,oy,ox,n] = sum_{r,s,c} x[b, f(oy*stride+r-pad_t), f(ox*stride+s-pad_l), c] * w[n][r][s][c]
 *                  + bias[n] + rowbias[b*rowbias_ld + n] + residual[b,oy,ox,n]      (+ y when accumulate)
 * f = identity | v>>1 (upsample=1, H/W are the stored low-res dims) | v/2 for even v only (dilate=1: the dgrad
 * of a stride-2 conv).  w is packed [N][R][S][C] in dtype (ddpm_pack_weight).  dgrad = same call on dy with the
 * flipped/transposed pack and pad = R-1-pad.  out_mode: 0 NHWC dtype (pitch y_ld) | 1 NHWC fp32 | 3 NCHW fp32.
 * splits > 1 splits K over blocks and reduces in-launch (for layers with few output tiles): splitk_ws holds
 * max(ceil(M/128)*ceil(N/128)*16384, ceil(M/64)*ceil(N/64)*4096)*splits floats and splitk_cnt one zero-initialised counter
 * per 64x64 output tile (left zero) — the library picks the tile size.  splits == 2 is an OFFER to the small-grid kernel (at most
 * 128 tiles of 64x64): it takes 2, 4 or 8 K runs per tile with tiles x runs <= 256, so for splits == 2 splitk_ws must hold at
 * least 256*4096 floats (4 MiB) as well.
 * Operand limit: x (B*H*W stored pixels of pitch x_ld) and w; beyond it the call returns 1.  One form has none: 3x3 / stride 1 /
 * pad 1 on bf16 with C == 8, N % 16 == 0, N <= 128, H and W multiples of 16, at least 16384 output pixels and neither row bias,
 * residual nor accumulate (the few-input-channel edge kernel) reads x through 64-bit pointers. */
int ddpm_conv2d_nhwc(const void* x, long long x_ld, const void* w, void* y, long long y_ld,
                     const float* bias, const float* rowbias, long long rowbias_ld,
                     const void* residual, long long res_ld,
                     int B, int H, int W, int C, int Ho, int Wo, int N, int R, int S,
                     int stride, int pad_t, int pad_l, int upsample, int dilate,
                     int accumulate, int out_mode, int splits, float* splitk_ws, unsigned* splitk_cnt,
                     int dtype, void* stream);

/* convolution_backward w.r.t. the weight (autograd of the sites above), into a PACKED gradient [Nreal][R][S][Creal]:
 *   dw[n][r][s][c] += sum_{b,oy,ox} dy[b,oy,ox,n] * x[b, f(..), f(..), c]      n < Nreal, c < Creal
 * dy has N (>= Nreal) channels, x has C (>= Creal) channels (zero padding beyond the real counts).  The reduction over
 * B*Ho*Wo is cut into `splits` slices that run as separate workgroups:
 *   slab_stride == 0: every slice adds into dw with fp32 atomics (dw must be zero-filled / hold earlier contributions);
 *   slab_stride  > 0: slice s STORES its partial at dw + s*slab_stride (floats) — `splits` must then equal
 *                     ddpm_wgrad_effective_splits(B*Ho*Wo, splits, dtype) so that every copy is written — and
 *                     ddpm_wgrad_reduce sums the copies in a fixed order (bit-deterministic gradients).
 *                     table[i] = {src address of copy 0, dst address, floats, copies, stride}.
 * ddpm_wgrad_unpack rewrites all layers' packed gradients into the parameter layout [n][c][r][s] in one launch:
 * descs[i] = {src offset in gpack, dst offset in gflat (floats), N, C, R*S} as int64 (R*S = 1: plain segment copy);
 * every value is multiplied by `scale` (1/world_size after the data-parallel sum all-reduce of gpack).
 * Operand limit (ddpm_conv2d_wgrad_nhwc): dy ([B*Ho*Wo][N], pitch dy_ld) and x (B*H*W stored pixels of pitch x_ld). */
int ddpm_conv2d_wgrad_nhwc(const void* dy, long long dy_ld, const void* x, long long x_ld, float* dw, long long slab_stride,
                           int B, int H, int W, int C, int Creal, int Ho, int Wo, int N, int Nreal, int R, int S,
                           int stride, int pad_t, int pad_l, int upsample, int splits, int dtype, void* stream);

int ddpm_wgrad_effective_splits(int K, int splits, int dtype);

/* The same gradient for the 3x3 / stride 1 / pad 1 sites (ResidualBlock.conv1 / conv2, ddpm_torch/models/unet.py:76,79), bf16, by a
 * patch-stationary kernel: a block keeps a 64 x 32 x 9-tap output tile and walks 16x16 pixel patches whose dy tile and x halo are
 * staged in LDS once for all nine taps; the reduction over pixels is cut into few slices.  Also produces the bias gradient
 * dbias[n] = sum_{b,y,x} dy[b,y,x,n] (optional) from the dy fragments it reads anyway.
 *   slab_stride == 0: fp32 atomics into dw [Nreal][3][3][C] / dbias [Nreal];
 *   slab_stride  > 0: slice s stores at dw + s*slab_stride (and dbias + s*bias_stride); all ddpm_conv3x3_wgrad_splits(...)
 *                     copies are written in full and ddpm_wgrad_reduce sums them in a fixed order (deterministic).
 * C % 32 == 0, N % 8 == 0 and H = W in {4, 8} or H, W multiples of 16; otherwise DDPM_ERR_SHAPE (use ddpm_conv2d_wgrad_nhwc).
 * splits <= 0: chosen by the library.
 * Operand limit: dy (B*H*W pixels of pitch dy_ld) and x (B*H*W pixels of pitch x_ld; the _up_ entry: B*(H/2)*(W/2)). */
int ddpm_conv3x3_wgrad_splits(int B, int H, int W, int C, int N, int splits);
int ddpm_conv3x3_wgrad_nhwc(const void* dy, long long dy_ld, const void* x, long long x_ld, float* dw, long long slab_stride,
                            float* dbias, long long bias_stride, int B, int H, int W, int C, int N, int Nreal, int splits,
                            int dtype, void* stream);
/* ... of the conv inside an Upsample block (`nn.Upsample(scale_factor=2, mode="nearest")` then the 3x3 conv, ddpm_torch/models/unet.py:199-202, through autograd): H, W are the
 * OUTPUT image (dy's), x is the block's input stored at H/2 x W/2; the kernel gathers stored pixel (y >> 1, x >> 1).  ddpm_conv3x3_wgrad_splits
 * is asked with the same (output) H, W. */
int ddpm_conv3x3_wgrad_up_nhwc(const void* dy, long long dy_ld, const void* x, long long x_ld, float* dw, long long slab_stride,
                               float* dbias, long long bias_stride, int B, int H, int W, int C, int N, int Nreal, int splits,
                               int dtype, void* stream);

/* Weight (and bias) gradient of a 1x1 / stride-1 convolution — autograd of F.conv2d (ddpm_torch/modules.py:120-123) at the attention
 * projections and skip connections (ddpm_torch/models/unet.py:36-37,41 `AttentionBlock.project_in/out/skip`, :80 `ResidualBlock.skip`) — by the slab kernel of csrc/wgrad1x1.hip (bf16):
 *     dW[n][c] = sum_p dy[p][n] * x[p][c]      db[n] = sum_p dy[p][n]      p over the P = B*H*W pixels
 * ddpm_conv1x1_wgrad_splits returns the number of slab copies the kernel writes for this geometry (0: not covered, use
 * ddpm_conv2d_wgrad_nhwc); slice s STORES its partials at dw + s*slab_stride ([N][C] fp32) and dbias + s*bias_stride (dbias may be
 * NULL); ddpm_wgrad_reduce sums the copies in a fixed order.
 * Operand limit: dy ([P][N], pitch dy_ld) and x ([P][C], pitch x_ld). */
int ddpm_conv1x1_wgrad_splits(int P, int C, int N);
int ddpm_conv1x1_wgrad_nhwc(const void* dy, long long dy_ld, const void* x, long long x_ld, float* dw, long long slab_stride,
                            float* dbias, long long bias_stride, int P, int C, int N, int splits, int dtype, void* stream);

int ddpm_wgrad_reduce(const long long* table, int n_tensors, void* stream);

int ddpm_wgrad_unpack(const float* gpack, float* gflat, const long long* descs, int n_tensors, float scale, void* stream);
/* ... the same pass, also producing the sum of squares of everything it writes: the global gradient norm of nn.utils.clip_grad_norm_
 * (ddpm_torch/utils/train.py:159) without another read of all gradients.  total_sq: ddpm_mt_sumsq_slots(n_tensors) floats; every block
 * stores its partial in its own slot behind the 64-float bank and a second launch adds the slots in a FIXED order: on return
 * (stream-ordered) total_sq[0] is the sum and lanes 1..63 are zero — bit-deterministic, so data-parallel replicas holding identical
 * gradients derive the identical clip coefficient (fp32 atomics into the bank, as before round 5, let them drift apart by ulps).
 * total_sq_floats: the capacity of total_sq in floats; DDPM_ERR_SHAPE when it is below ddpm_mt_sumsq_slots(n_tensors) (the buffer was a
 * 64-float bank before round 5: a caller that still passes one is refused instead of being written past). */
int ddpm_wgrad_unpack_sumsq(const float* gpack, float* gflat, const long long* descs, int n_tensors, float scale, float* total_sq,
                            long long total_sq_floats, void* stream);

/* F.linear (modules.py:58-59; unet.py:77,123,125) and torch.einsum in AttentionBlock.qkv (unet.py:46,50):
 *   C[b][m][n] = alpha * sum_k A[b][m][k] * B[b][n][k] + bias[n] + residual[b][m][n]   (+ C when accumulate)
 * a_trans/b_trans = 1: the operand is stored [k][m] / [k][n].  out_mode: 0 dtype | 1 fp32 | 2 fp32 atomic add.
 * Operand limit: A and B PER BATCH (one [rows][cols] matrix of pitch a_ld / b_ld); the batch strides are 64-bit, so the batches
 * together may span any size. */
int ddpm_gemm(const void* a, long long a_ld, long long a_bs, int a_trans,
              const void* b, long long b_ld, long long b_bs, int b_trans,
              void* c, long long c_ld, long long c_bs,
              const float* bias, const void* residual, long long res_ld, long long res_bs,
              int M, int N, int K, int batch, float alpha, int accumulate, int out_mode, int splits,
              int dtype, void* stream);

/* Fused single-head attention forward (inference path) — replaces the three products of AttentionBlock.forward
 * (ddpm_torch/models/unet.py:41-52: einsum("bchw,bcHW->bhwHW") * C**-0.5, softmax over the key positions, einsum with v)
 * for a packed projection buffer qkv[B][L][ld] with q at channel 0, k at channel C and v at channel 2C:
 *     out[b][i][:] = sum_j softmax_j(q[b][i] . k[b][j] * scale) v[b][j]        (out pitch out_ld, bf16)
 * The L x L logits stay on chip (LDS / registers).  bf16 only, C in {128, 256}, L a multiple of 128; anything else returns
 * DDPM_ERR_SHAPE and the caller keeps ddpm_gemm + ddpm_softmax_fwd + ddpm_gemm.
 * Operand limit: q, k and v of one sample ((L - 1) * ld + C elements each); the samples' bases are 64-bit. */
int ddpm_attention_fwd(const void* qkv, long long ld, void* out, long long out_ld, int B, int L, int C, float scale,
                       int dtype, void* stream);

/* Attention for training, and for every geometry ddpm_attention_fwd does not serve (ddpm_torch/models/unet.py:41-52 and its autograd
 * backward): same packed qkv layout.  The forward also writes lse[b][i] = log sum_j exp(q_i . k_j * scale) (fp32, [B][L]; may be NULL
 * for inference); the backward rebuilds the probabilities from q, k and lse on chip — no L x L tensor is ever written — and produces
 *     dV = P^T dO      dS = P o (dO V^T - D),  D[i] = sum_c dO[i][c] O[i][c]      dQ = dS K * scale      dK = dS^T Q * scale
 * into the packed gradient buffer dqkv[B][L][dqkv_ld] (dq at channel 0, dk at C, dv at 2C).  dvec: [B][L] fp32 workspace (receives D).
 * bf16 only; L <= 256 with L % 16 == 0 (the reference attends at 16x16 and below); C <= 512 with C % 32 == 0; else DDPM_ERR_SHAPE.
 * Operand limit: qkv of ONE sample, L * ld * 2 <= 0x7ffffff0 bytes, and in the backward d_o likewise, L * do_ld * 2 (do_ld >= C); the
 * samples' bases are 64-bit, and o, out and dqkv are addressed with 64-bit pointers. */
int ddpm_attention_fwd_lse(const void* qkv, long long ld, void* out, long long out_ld, float* lse, int B, int L, int C, float scale,
                           int dtype, void* stream);
int ddpm_attention_bwd(const void* qkv, long long ld, const void* o, long long o_ld, const void* d_o, long long do_ld,
                       const float* lse, float* dvec, void* dqkv, long long dqkv_ld, int B, int L, int C, float scale,
                       int dtype, void* stream);

/* The same pair at ANY token count (csrc/attention_stream.hip): the other side of the score matrix is streamed through LDS in tiles
 * with an online softmax, so no L x L object exists and no L is a memory row.  Parameter lists, layouts, null / alignment / pitch rules
 * and status codes are those of the pair above; lse may be NULL in the forward.  bf16 only (DDPM_ERR_DTYPE); any L >= 1 with
 * L * ld * 2 bytes within the buffer descriptors' range (0x7ffffff0), C <= 512 with C % 32 == 0 (else DDPM_ERR_SHAPE).  No allocation,
 * synchronisation or attribute call: safe as the first call inside a stream capture.  The backward uses no atomics and no split
 * accumulation: a repeated call is bit-identical.  Reads only [B][L][C] of each operand, writes only [B][L][C] of each output. */
int ddpm_attention_stream_fwd(const void* qkv, long long ld, void* out, long long out_ld, float* lse, int B, int L, int C, float scale,
                              int dtype, void* stream);
int ddpm_attention_stream_bwd(const void* qkv, long long ld, const void* o, long long o_ld, const void* d_o, long long do_ld,
                              const float* lse, float* dvec, void* dqkv, long long dqkv_ld, int B, int L, int C, float scale,
                              int dtype, void* stream);

/* Multi-head attention at any token count: the streaming pair with a head index (the same kernels; the pair above is heads = 1 of
 * this code, bit for bit).  d = C / heads.  Head h of q, k and v is channels [h d, (h + 1) d) of its third of the packed buffer — q at
 * channel 0, k at C, v at 2C, i.e. qkv.chunk(3) followed by a split of each third into heads (the ordering of ADM's QKVAttention):
 *     out[b][i][h d + c] = sum_j softmax_j(q_h[b][i] . k_h[b][j] * scale) v_h[b][j][c]
 * out, o, d_o and the thirds of dqkv use the same head layout.  lse and dvec are [B][heads][L] fp32 (lse may be NULL in the forward).
 * The caller passes scale: 1 / sqrt(d) for the usual attention.  Validation, on the host before any launch: everything the streaming
 * pair validates with its status codes (pitch rules on the full 3C / C rows, C <= ld / 3), and DDPM_ERR_SHAPE unless heads >= 1,
 * C % heads == 0, d % 32 == 0, d <= 512 and B * heads <= 65535; bf16 only.  C itself is not bounded by 512.  The kernel bucket
 * follows d as the streaming pair's follows C (d = 32 runs in the 64-channel bucket).  No allocation, synchronisation or attribute
 * call; no atomics or split accumulation (a repeated backward is bit-identical); a head reads only its own [L][d] of each operand and
 * writes only its own [L][d] of each output.
 * Operand limit (this pair and the streaming pair above), per sample: L * ld * 2 <= 0x7ffffff0 bytes for qkv, and in the backward
 * also L * o_ld * 2 and L * do_ld * 2 for o and d_o; the samples' bases are 64-bit. */
int ddpm_attention_mh_fwd(const void* qkv, long long ld, void* out, long long out_ld, float* lse, int B, int L, int C, int heads,
                          float scale, int dtype, void* stream);
int ddpm_attention_mh_bwd(const void* qkv, long long ld, const void* o, long long o_ld, const void* d_o, long long do_ld,
                          const float* lse, float* dvec, void* dqkv, long long dqkv_ld, int B, int L, int C, int heads, float scale,
                          int dtype, void* stream);

/* Operand limit of the four GroupNorm entries below: every activation operand (x, y; dy, dx, add) must hold fewer than 2^31 elements,
 * (B*HW - 1) * ld + C < 2^31, else 1 (bad shape) before any launch.  Up to that size the library picks a form whose indexing reaches
 * the operand (the LDS-staged forms are used only while one sample's slice of every operand ends within 0x7ffffff0 bytes).
 * nn.GroupNorm(32, C, eps=1e-6) -> SiLU -> Dropout(p) (unet.py:18-20,15,81,85-87,139-140; :57 without SiLU):
 *   y = drop(silu((x - mean_g) * rstd_g * gamma_c + beta_c)),  biased variance over (C/G)*HW elements.
 * stats (optional) receives [B][G][2] = (mean, rstd) for the backward.  workspace: ddpm_gn_workspace_floats().
 * Dropout keep-mask = hash(seed, linear NHWC index) (see ddpm_dropout_mask); scale 1/(1-p).  seed_dev (optional device
 * word): the effective seed is seed + *seed_dev — a captured hipGraph then draws a fresh mask on every replay.
 * A dropped element is exactly 0 whatever its value (a select, not a product); a NaN or inf in a group makes every kept element of
 * that (sample, group) and its statistics non-finite, and nothing else.
 * Statistics are accumulated about a per-group pivot (the median of three elements of the group), so |mean| >> std keeps full
 * accuracy. */
int ddpm_groupnorm_silu_fwd(const void* x, long long x_ld, void* y, long long y_ld, const float* gamma, const float* beta,
                            float* stats, float* workspace, int B, int HW, int C, int G, float eps, int silu,
                            float drop_p, unsigned long long seed, const unsigned long long* seed_dev, int dtype, void* stream);
/* backward of the above: dx (+= when accumulate), dgamma/dbeta += (fp32 atomics).  dx_colsum (optional): receives the per-sample
 * channel sums of dx, dx_colsum[b*colsum_ld + c] = sum_pixels dx[b,:,c] — the gradient of the per-sample time bias that was added
 * in front of this GroupNorm (ddpm_torch/models/unet.py:86); the buffer must be zero on entry (paths without the fused sum add into it).
 * add (optional, NHWC with pitch add_ld): a second gradient contribution added to dx in the same pass — the identity branch of the
 * residual connections (unet.py:60,89): dx = gn_backward(dy) + add  (no separate fan-in add launch). */
int ddpm_groupnorm_silu_bwd(const void* x, long long x_ld, const void* dy, long long dy_ld, void* dx, long long dx_ld,
                            const float* gamma, const float* beta, const float* stats, float* dgamma, float* dbeta,
                            float* workspace, int B, int HW, int C, int G, int silu, float drop_p, unsigned long long seed,
                            const unsigned long long* seed_dev, int accumulate, float* dx_colsum, long long colsum_ld,
                            const void* add, long long add_ld, int dtype, void* stream);
long long ddpm_gn_workspace_floats(int B, int HW, int C, int G, int dtype);

/* Scale-shift norm (AdaGN, `use_scale_shift_norm` of the Improved-DDPM / ADM residual block): the same kernels with a per-sample affine,
 *   y = drop(silu(xhat * g_eff + b_eff)),   g_eff[b,c] = gamma[c] * (1 + s[b,c]),   b_eff[b,c] = beta[c] * (1 + s[b,c]) + h[b,c],
 * xhat = (x - mean_g) * rstd_g.  mod: fp32, row b at mod + b*mod_ld, scale s in columns [0, C), shift h in [C, 2C); mod_ld >= 2C is
 * otherwise arbitrary and the columns past 2C are never read.  Everything else (stats, workspace — sized by ddpm_gn_workspace_floats —,
 * dropout, seed_dev, pitches) is ddpm_groupnorm_silu_fwd's; the products are formed in fp32 as written, so with mod == 0 the result,
 * stats included, equals the plain entry point's bit for bit.  A sample's row of mod reaches that sample only.
 * Validation on the host before any launch: everything the plain entry point checks, DDPM_ERR_NULL for a null mod, DDPM_ERR_SHAPE
 * for mod_ld < 2C. */
int ddpm_groupnorm_mod_silu_fwd(const void* x, long long x_ld, void* y, long long y_ld, const float* gamma, const float* beta,
                                float* stats, float* workspace, int B, int HW, int C, int G, float eps, int silu,
                                float drop_p, unsigned long long seed, const unsigned long long* seed_dev,
                                const float* mod, long long mod_ld, int dtype, void* stream);
/* backward of the above.  With t = g_eff*xhat + b_eff, dz = dy * keep/(1-p) * silu'(t), A[b,c] = sum_p dz*xhat, D[b,c] = sum_p dz:
 *   dx = rstd * (dz*g_eff - xhat*c1 - c2)   (c1, c2: group means of dz*g_eff*xhat, dz*g_eff; accumulate / add / dx_colsum as in the plain
 *   backward — dx_colsum here is the per-sample share of the gradient of a bias added in front of the norm, conv1.bias in the block),
 *   dgamma[c] += sum_b A*(1 + s),  dbeta[c] += sum_b D*(1 + s)   (fp32 atomics, as in the plain backward),
 *   dmod[b*dmod_ld + c] = gamma[c]*A + beta[c]*D,  dmod[b*dmod_ld + C + c] = D   (d/d scale, d/d shift).
 * Each of the 2C gradient columns of a dmod row is OVERWRITTEN by one plain store from the one block that completes the sample's
 * channel sums: no atomics, nothing accumulated, bit-identical from run to run; columns past 2C are not touched.  No pass over
 * x, dy or dx beyond the plain backward's.  With mod == 0, dx equals the plain backward's bit for bit.
 * Validation: as the forward, plus DDPM_ERR_NULL for a null dmod and DDPM_ERR_SHAPE for dmod_ld < 2C. */
int ddpm_groupnorm_mod_silu_bwd(const void* x, long long x_ld, const void* dy, long long dy_ld, void* dx, long long dx_ld,
                                const float* gamma, const float* beta, const float* stats, float* dgamma, float* dbeta,
                                float* workspace, int B, int HW, int C, int G, int silu, float drop_p, unsigned long long seed,
                                const unsigned long long* seed_dev, int accumulate, float* dx_colsum, long long colsum_ld,
                                const void* add, long long add_ld, const float* mod, long long mod_ld, float* dmod, long long dmod_ld,
                                int dtype, void* stream);

/* get_timestep_embedding (ddpm_torch/functions.py:10-26): out[b] = cat(sin(t_b f), cos(t_b f)) (zero pad if dim odd);
 * freqs[dim/2] = exp(-i ln(1e4)/(dim/2 - 1)) is supplied by the host in fp32. */
int ddpm_timestep_embedding(const long long* t, const float* freqs, float* out, int B, int dim, void* stream);

/* layout / packing helpers (no reference counterpart: the NHWC + packed-weight layout is this library's).
 * ddpm_nchw_to_nhwc: y[b][p][c] = x[b][c][p] for c < C, 0 for C <= c < Cp.  No operand limit (64-bit element indices). */
int ddpm_nchw_to_nhwc(const float* x, void* y, int B, int C, int HW, int Cp, int dtype, void* stream);
int ddpm_pack_weight(const float* w, void* w_fwd /*[N][R][S][Cp]*/, void* w_dgrad /*[C][R][S][Np], taps flipped*/,
                     int N, int C, int R, int S, int Cp, int Np, int dtype, void* stream);

/* every layer's pack in one launch: descs[i] = {w, w_fwd, w_dgrad (or 0), N, C, R (== S), Cp, Np} as int64 */
int ddpm_pack_weight_multi(const long long* descs, int n_tensors, int dtype, void* stream);

/* GaussianDiffusion.q_sample (ddpm_torch/diffusion.py:92-97): xt = sqrt_ab[t]*x0 + sqrt_1mab[t]*noise  (fp32, [B][n]).
 * T = table length: a sample whose t is outside [0, T) is filled with NaN (the reference's gather raises, :83). */
int ddpm_q_sample(const float* x0, const float* noise, const long long* t, const float* sqrt_ab, const float* sqrt_1mab,
                  float* xt, int B, int n, int T, void* stream);
/* flat_mean((target - pred)^2) (diffusion.py:239, functions.py:99-101) and its gradient w.r.t. pred */
int ddpm_mse_fwd(const float* pred, const float* target, float* loss, int B, int n, void* stream);
int ddpm_mse_bwd(const float* pred, const float* target, const float* gloss, float* gpred, int B, int n, void* stream);
/* out[0] = sum_i x[i]*w[i], one block, fixed order: the batch mean of the per-sample losses (utils/train.py:151 `loss.mean()`) */
int ddpm_weighted_sum_f32(const float* x, const float* w, float* out, int n, void* stream);
/* C[m][n] = sum_k A[k][m] * B[k][n] in fp32 for short reductions (K = the batch): the weight gradients of the time-embedding path —
 * autograd of F.linear (ddpm_torch/modules.py:58-59) at ResidualBlock.fc (models/unet.py:77,86) and UNet.embed (:122-126): dW = d(out)^T in.
 * A is [K][lda], B is [K][ldb], C is [M][ldc]; plain stores in a fixed order (bit-deterministic). */
int ddpm_atb_f32(const float* a, long long lda, const float* b, long long ldb, float* c, long long ldc, int M, int N, int K, void* stream);
/* p_mean_var + p_sample_step (diffusion.py:107-158; ddim.py inherits it): one fused update
 *   x0 = clamp(recip[t]*x_t - recip_m1[t]*out)   (mean_type 0 = eps; 1: x0 = out; 2: out is the mean)
 *   x_prev = coef1[t]*x0 + coef2[t]*x_t + 1[t>0]*exp(0.5*logvar[t])*z ;  pred_x0 optional.
 * The clamp propagates NaN like torch.clamp; T = table length, t outside [0, T) poisons the sample with NaN. */
int ddpm_p_sample_step(const float* x_t, const float* model_out, const float* z, const long long* t,
                       const float* sqrt_recip_ab, const float* sqrt_recip_m1_ab, const float* post_coef1, const float* post_coef2,
                       const float* logvar, float* x_prev, float* pred_x0, int B, int n, int mean_type, int clip, int T, void* stream);
/* Variational-bound term L_t in bits per dimension — ddpm_torch/diffusion.py:203-215 `_loss_term_bpd` (loss_type = "kl", :222-224;
 * `calc_all_bpd`, :251-267): per sample b the mean over the n elements of KL(q(x_{t-1}|x_t,x_0) || p(x_{t-1}|x_t)) / ln 2 for t[b] > 0
 * (functions.py:30-36 `normal_kl`, both log-variances table entries) or of the discretized-Gaussian decoder NLL / ln 2 for t[b] = 0
 * (functions.py:39-65).  The model mean is derived from the network output as in ddpm_p_sample_step (mean_type 0 eps | 1 x_0 | 2 mean;
 * clip as `clip_denoised`); pred_x0 (may be null) receives the x_0 estimate.  Tables: fp32, length T; t outside [0, T) poisons the row.
 * ddpm_vlb_terms_bwd: gout[b][i] = gloss[b] * d loss[b] / d model_out[b][i] (clip_denoised = False, as `train_losses` calls it). */
int ddpm_vlb_terms(const float* x_0, const float* x_t, const float* model_out, const long long* t,
                   const float* sqrt_recip_ab, const float* sqrt_recip_m1_ab, const float* post_coef1, const float* post_coef2,
                   const float* post_logvar, const float* model_logvar, float* loss, float* pred_x0,
                   int B, int n, int mean_type, int clip, int T, void* stream);
int ddpm_vlb_terms_bwd(const float* x_0, const float* x_t, const float* model_out, const long long* t,
                       const float* sqrt_recip_ab, const float* sqrt_recip_m1_ab, const float* post_coef1, const float* post_coef2,
                       const float* post_logvar, const float* model_logvar, const float* gloss, float* gout,
                       int B, int n, int mean_type, int T, void* stream);
/* One step of `calc_all_bpd` (ddpm_torch/diffusion.py:252-268) behind the network.  Per sample b with 0 <= t[b] < T:
 *   losses[b*ld + t[b]] = the value ddpm_vlb_terms computes (same model mean, same operation order; decoder 0 = the discretized Gaussian
 *                         at t = 0, decoder 1 = the toy pipeline's continuous Gaussian, functions.py:68-72: 0.5 (d^2 e^-logvar + ln 2pi + logvar))
 *   mses[b*ld + t[b]]   = mean_i (pred_x_0[b][i] - x_0[b][i])^2, pred_x_0 clipped to [-1, 1] when `clip` is set and never stored
 * from one pass over x_0, x_t, model_out.  A sample whose t is outside [0, T) writes nothing (the caller pre-fills both tables with NaN).
 * ld >= T is the row pitch of both tables.  No atomics, fixed reduction order: repeated launches are bit-identical.
 * ddpm_bpd_finish: prior[b] = mean_i normal_kl(sqrt_ab_last * x_0, log_1m_ab_last, 0, 0) / ln 2 (:245-250),
 *                  total[b] = (sum_t losses[b*ld + t], fixed order) + prior[b]. */
int ddpm_bpd_terms(const float* x_0, const float* x_t, const float* model_out, const long long* t,
                   const float* sqrt_recip_ab, const float* sqrt_recip_m1_ab, const float* post_coef1, const float* post_coef2,
                   const float* post_logvar, const float* model_logvar, float* losses, float* mses,
                   int B, int n, int ld, int mean_type, int clip, int decoder, int T, void* stream);
int ddpm_bpd_finish(const float* x_0, const float* losses, float* prior, float* total, int B, int n, int T, int ld,
                    float sqrt_ab_last, float log_1m_ab_last, void* stream);
/* Learned reverse-process variance (model_var_type "learned", diffusion.py:111-114, and "learned-range", Nichol & Dhariwal 2021 eq. 15).
 * model_out is [B][2n] fp32: the mean output (eps / x_0 / mean by mean_type, as above) at b*2n + i and v at b*2n + n + i, both read in place.
 * The model log-variance of an element is
 *   var_mode 1: v;    var_mode 2: f*lv_max[t] + (1 - f)*lv_min[t] with f = (v + 1)/2, not clamped (each product and sum rounded on its
 *   own: v = +1 / -1 give the table entries to the bit);    var_mode 0 (step only): the table entry logvar_lo[t], v ignored.
 * Model mean, KL, discretized decoder (decoder 0 only), operation order and reduction trees are those of the fixed-variance siblings
 * with that log-variance in the place of model_logvar[t].  fp32, no atomics, fixed reduction order: repeated launches are bit-identical.
 * Tables have length T; a sample whose t is outside [0, T) is poisoned with NaN (step, terms, loss: every output of the sample) or writes
 * nothing (ddpm_bpd_terms_lv), and no table is read for it.
 * ddpm_p_sample_step_lv: ddpm_p_sample_step's update and noise mask.  var_mode 0: logvar_lo = the fixed table (logvar_hi may be NULL);
 *   1: both may be NULL; 2: logvar_lo = lv_min (posterior_logvar_clipped), logvar_hi = lv_max (the "fixed-large" table).  pred_x0 may be
 *   NULL; x_prev may be x_t (an element is read once, then written).
 * ddpm_vlb_terms_lv / ddpm_bpd_terms_lv: ddpm_vlb_terms (loss [B], optional pred_x0) and ddpm_bpd_terms (column t[b] of the [B][ld]
 *   tables; the three row layouts: a wave per row for n <= 64, 256 threads, 1024 threads with 16-byte loads where the four row bases are
 *   16-byte aligned) with var_mode 1 | 2; post_logvar is the true posterior's table and lv_min, logvar_max (NULL allowed for var_mode 1) lv_max.
 * ddpm_learned_loss: one pass over x_0, x_t, model_out, target (all [B][n] but model_out), clip_denoised = False:
 *   loss[b]        = w_mse * mean_i (out_mean - target)^2 + w_vlb * L_t(out_mean, v)                     (L_t in bits/dim)
 *   gout[b][i]     = gloss[b] * (w_mse * 2 (out_mean - target) / n + (detach_mean ? 0 : w_vlb * dL_t/d out_mean))       i < n
 *   gout[b][n + i] = gloss[b] * w_vlb * dL_t/dv            (through logvar; var_mode 2: times (lv_max[t] - lv_min[t]) / 2)
 *   The backward differentiates the forward's own expressions (tanh CDF, floor, open tails).  gout NULL: the loss alone (gloss unused).
 *   A weight of exactly 0 switches its term off: target may be NULL when w_mse = 0; with w_vlb = 0 the v half of gout is 0.0.
 *   (1, lambda, detach_mean 1) is the hybrid loss of eq. 16, (0, 1, 0) loss_type "kl" with its full gradient. */
int ddpm_p_sample_step_lv(const float* x_t, const float* model_out, const float* z, const long long* t,
                          const float* sqrt_recip_ab, const float* sqrt_recip_m1_ab, const float* post_coef1, const float* post_coef2,
                          const float* logvar_lo, const float* logvar_hi, float* x_prev, float* pred_x0,
                          int B, int n, int mean_type, int clip, int var_mode, int T, void* stream);
int ddpm_vlb_terms_lv(const float* x_0, const float* x_t, const float* model_out, const long long* t,
                      const float* sqrt_recip_ab, const float* sqrt_recip_m1_ab, const float* post_coef1, const float* post_coef2,
                      const float* post_logvar, const float* logvar_max, float* loss, float* pred_x0,
                      int B, int n, int mean_type, int clip, int var_mode, int T, void* stream);
int ddpm_bpd_terms_lv(const float* x_0, const float* x_t, const float* model_out, const long long* t,
                      const float* sqrt_recip_ab, const float* sqrt_recip_m1_ab, const float* post_coef1, const float* post_coef2,
                      const float* post_logvar, const float* logvar_max, float* losses, float* mses,
                      int B, int n, int ld, int mean_type, int clip, int decoder, int var_mode, int T, void* stream);
int ddpm_learned_loss(const float* x_0, const float* x_t, const float* model_out, const float* target, const long long* t,
                      const float* sqrt_recip_ab, const float* sqrt_recip_m1_ab, const float* post_coef1, const float* post_coef2,
                      const float* post_logvar, const float* logvar_max, const float* gloss, float* loss, float* gout,
                      int B, int n, int mean_type, int var_mode, int detach_mean, int T, float w_mse, float w_vlb, void* stream);
/* Class conditioning and classifier-free guidance (csrc/guidance.hip; Ho & Salimans 2022).  fp32; y and t are int64; every product and sum
 * is rounded on its own (no contraction) except the two fused operations of ddpm_p_sample_step's update.  Static LDS only, no atomics, no
 * allocation: each is capturable as a first call.  Status: a required pointer NULL DDPM_ERR_NULL; B, E, K1, n or T <= 0, K1 > 65535
 * (ddpm_class_embed_bwd), B > 65535 or mean_type outside 0..2 (ddpm_p_sample_step_cfg) DDPM_ERR_SHAPE; a pointer that is not a multiple of
 * its element size DDPM_ERR_ALIGN.
 * ddpm_class_embed_fwd: table is [K1][E], K1 = num_classes + 1, row K1 - 1 the null class (the label of a dropped or absent condition).
 *   pre[b] = t_emb[b] + table[y[b]],  s[b] = SiLU(pre[b]) with ddpm_silu_fwd's expression: s equals ddpm_silu_fwd(pre) bit for bit.
 *   t_emb, pre, s are [B][E].  A sample whose y[b] is outside [0, K1) gets NaN rows in pre and s, and no table row is read for it.
 * ddpm_class_embed_bwd: dtable[k][e] = sum of dpre[b][e] over the samples with y[b] == k, added in ascending b (a fixed order: repeated
 *   launches are bit-identical); a class without a sample gets 0.0.  Plain stores to every element of dtable [K1][E], so nothing the
 *   buffer held before survives.  A y[b] outside [0, K1) contributes nothing.
 * ddpm_p_sample_step_cfg: the sampling step on the guided combination of a doubled batch.  model_out2 is [2B][n]: rows [0, B) the
 *   conditional network output, rows [B, 2B) the unconditional one (eps, x_0 or mean alike: the two weights sum to one).
 *     g = scale * out_c + (1 - scale) * out_u      (1 - scale formed once in fp32; two products and one sum, three roundings)
 *   followed by exactly ddpm_p_sample_step's operations on g, tables, mean_type, clip, noise mask and T as there.  For finite inputs
 *   scale = 1 gives the bits of ddpm_p_sample_step on out_c and scale = 0 those on out_u (up to the sign of a zero network output).
 *   x_t is read from rows [0, B) of its buffer; x_prev is written to row b and, when dup != 0, also to row b + B of a [2B][n] buffer (the
 *   doubled state of the next network call).  x_prev may be x_t (an element is read once, then written; rows [B, 2B) are never read).
 *   z is [B][n]; pred_x0 ([B][n]) may be NULL.  A sample whose t is outside [0, T) gets NaN in every row written for it, no table is read
 *   for it and no other sample is touched.  A sample whose row bases are all 16-byte aligned is moved 16 bytes per lane with a scalar
 *   tail, any other one element-wise; both paths give the same bits. */
int ddpm_class_embed_fwd(const float* t_emb, const float* table, const long long* y, float* pre, float* s, int B, int E, int K1, void* stream);
int ddpm_class_embed_bwd(const float* dpre, const long long* y, float* dtable, int B, int E, int K1, void* stream);
int ddpm_p_sample_step_cfg(const float* x_t, const float* model_out2, const float* z, const long long* t,
                           const float* sqrt_recip_ab, const float* sqrt_recip_m1_ab, const float* post_coef1, const float* post_coef2,
                           const float* logvar, float scale, float* x_prev, float* pred_x0, int B, int n, int mean_type, int clip,
                           int dup, int T, void* stream);
/* subsequence.gather(0, t) (ddim.py:101) and t += delta (t.fill_ in diffusion.py:172, device-side for graph replay) */
int ddpm_gather_i64(const long long* idx, const long long* map, long long* out, int B, void* stream);
int ddpm_add_i64(long long* t, int B, long long delta, void* stream);
/* DDIM inversion (csrc/ddim.hip; Song et al. 2020 §4.3, eta = 0, eps parameterisation): one step of the sampler's ODE run from data to
 * noise.  With ab[i] = alphas_bar[subsequence[i]], ab_prev[i] = ab[i-1], ab_prev[0] = 1, step i takes the state from level i-1 to level i on
 * the network output at the timestep the sampling step i evaluates:
 *   x_next  = cx[t] * x + ce[t] * model_out        cx = sqrt(ab / ab_prev),  ce = sqrt(1 - ab) - sqrt(ab * (1 - ab_prev) / ab_prev)
 *   pred_x0 = sqrt_recip_ab_prev[t] * x - sqrt_recip_m1_ab_prev[t] * model_out        (optional: may be NULL; never clipped)
 * fp32, [B][n], tables of length S, two products and a sum per output, each rounded (no contraction).  ddpm_p_sample_step on the eta = 0
 * tables, the same t and the same model_out takes x_next back to x: the two share one index convention.  x_next may be x (an element is
 * read once, then written).  A sample whose t is outside [0, S) is filled with NaN and no other sample is touched.  A sample whose row
 * bases (x, model_out, x_next, pred_x0 at b * n) are all 16-byte aligned is moved 16 bytes per lane with a scalar tail, any other one
 * element-wise.  n >= 1.  Status: B, n or S <= 0 (or B > 65535) DDPM_ERR_SHAPE, a pointer that is not a multiple of its element size
 * DDPM_ERR_ALIGN.  Static LDS only, no atomics, no allocation: capturable as a first call. */
int ddpm_ddim_encode_step(const float* x, const float* model_out, const long long* t, const float* cx, const float* ce,
                          const float* sqrt_recip_ab_prev, const float* sqrt_recip_m1_ab_prev, float* x_next, float* pred_x0,
                          int B, int n, int S, void* stream);
/* Inpainting and image editing (csrc/inpaint.hip; RePaint: Lugmayr et al., CVPR 2022, Algorithm 1).  fp32; t is int64; every product and
 * sum is rounded on its own (no contraction) except the two fused operations of ddpm_p_sample_step's update.  Static LDS only, no atomics,
 * no allocation: each is capturable as a first call.
 * ddpm_p_sample_step_masked: one reverse step whose known region is re-noised from a source image.  x_t, z, x_known, e, x_prev are [B][n];
 *   model_out rows are out_pitch floats apart, out_pitch = n, or 2n for a 2C-channel network (mean output | v); var_mode 1 | 2 needs 2n and
 *   reads v at row[n + i] exactly as ddpm_p_sample_step_lv does, var_mode 0 with 2n reads the mean half alone (a DDIM on such a model).
 *   mask is [mask_rows][hw], mask_rows = 1 (one mask for the batch) or B, n % hw == 0: element i of sample b uses
 *   m = mask[mask_rows == 1 ? 0 : b][i % hw] (the mask is broadcast over channels), values in [0, 1], 1 = keep the known pixel, 0 = generate.
 *     u = x_prev of ddpm_p_sample_step (var_mode 0, logvar_lo the fixed table) / ddpm_p_sample_step_lv (var_mode 1 | 2, logvar_lo = lv_min,
 *         logvar_hi = lv_max) on the same x_t, model_out, z, t, tables, mean_type, clip: the same coefficients, noise mask 1[t>0],
 *         expf(0.5f * lv) and variance policy, so the same bits
 *     k = sqrt_ab_prev[t] * x_known + sqrt_1mab_prev[t] * e                  (two products and one sum, each rounded)
 *     x_prev = u where m == 0;  k where m == 1;  m * k + (1 - m) * u otherwise (1 - m formed once; two products and a sum, three roundings)
 *   The two exact cases are selects: NaN in x_known or e under m == 0, or in x_t, model_out or z under m == 1, does not reach the output.
 *   sqrt_ab_prev[t] = sqrt(ab[t-1]), sqrt_1mab_prev[t] = sqrt(1 - ab[t-1]) with ab[-1] = 1: the level the step arrives at, so at t = 0 the
 *   tables give 1 * x_known + 0 * e and the known region of the final image is the source image itself (up to the sign of a zero).
 *   There is no pred_x0 output.  x_prev may be x_t (an element is read once, then written, by one lane).  A sample whose t is outside
 *   [0, T) gets a row of NaN, no table is read for it and no other sample is touched.  grid = (column blocks, B).  A sample whose row bases
 *   (x_t, the mean half, the v half when read, z, x_known, e, x_prev and its mask row) are all 16-byte aligned, with hw % 4 == 0, is moved
 *   16 bytes per lane, any other one element-wise; both paths give the same bits.
 *   Status: a required pointer NULL DDPM_ERR_NULL (logvar_lo may be NULL in var_mode 1 only, logvar_hi is required in var_mode 2 only, as
 *   in ddpm_p_sample_step_lv); B, n, hw or T <= 0, B > 65535, n % hw != 0, mask_rows not in {1, B}, out_pitch not in {n, 2n}, var_mode 1 | 2
 *   with out_pitch != 2n, mean_type or var_mode outside 0..2 DDPM_ERR_SHAPE; a pointer that is not a multiple of its element size
 *   DDPM_ERR_ALIGN.
 * ddpm_q_jump: the forward process across j levels, x_out = ja[t] * x + jb[t] * z (two products and a sum, each rounded), with t the index
 *   the state ARRIVES at: ja[i] = sqrt(ab[i] / ab[i-j]), jb[i] = sqrt(1 - ab[i] / ab[i-j]), formed in fp64 on the host (the ratio of two
 *   fp32 table entries would lose about three digits of 1 - a at small betas).  x, z, x_out are [B][n], the tables have length T.  x_out may
 *   be x (ddpm_q_sample cannot serve: its operands are restrict-qualified and it has no 16-byte path).  Bad t, the 16-byte and the
 *   element-wise path (a scalar tail after n / 4 * 4 elements) and the status codes are those of the masked step. */
int ddpm_p_sample_step_masked(const float* x_t, const float* model_out, const float* z, const float* x_known, const float* e,
                              const float* mask, const long long* t, const float* sqrt_recip_ab, const float* sqrt_recip_m1_ab,
                              const float* post_coef1, const float* post_coef2, const float* logvar_lo, const float* logvar_hi,
                              const float* sqrt_ab_prev, const float* sqrt_1mab_prev, float* x_prev, int B, int n, int hw,
                              int mask_rows, int out_pitch, int mean_type, int clip, int var_mode, int T, void* stream);
int ddpm_q_jump(const float* x, const float* z, const long long* t, const float* ja, const float* jb, float* x_out, int B, int n, int T,
                void* stream);
/* Spherical interpolation of latents (Song et al. 2020 eq. 67), per pair p over the whole flattened sample: a, b [P][n], alpha [K],
 * out [P][K][n], fp32.
 *   c = clamp(<a,b> / (|a| |b|), -1, 1),  th = acos(c)
 *   out[p][k] = w0 * a[p] + w1 * b[p],   (w0, w1) = (sin((1 - alpha[k]) th), sin(alpha[k] th)) / sin(th)
 * Degenerate rule: when 1 - |c| < 1e-6 (nearly parallel or antiparallel) or c is not finite (a zero operand, an overflowing norm, NaN
 * in the pair) the weights are the linear ones, (w0, w1) = (1 - alpha[k], alpha[k]).  There is no other special case: NaN in an operand
 * reaches the outputs through the multiplies, and only those of its own pair.
 * Two passes, no atomics: pass one writes (<a,b>, |a|^2, |b|^2) of every 2048-element chunk of every pair to ws (summed in double, stored
 * as a (hi, lo) pair of floats each), pass two adds a pair's chunks up in double in a fixed order, forms the 2 K weights in double and writes out = fma(w0, a, w1 * b) — repeated launches are
 * bit-identical, and a pair is spread over ceil(n / 2048) workgroups in both passes.  ws: ddpm_slerp_workspace_floats(P, n) floats
 * (6 * P * ceil(n / 2048); 0 when P or n is 0, -1 when either is negative), overwritten by every call.  16-byte accesses when n % 4 == 0 and
 * a, b, out are 16-byte aligned, element-wise otherwise.  Status: P, K or n <= 0 (or P > 65535) DDPM_ERR_SHAPE, a pointer that is not a
 * multiple of 4 DDPM_ERR_ALIGN.  Static LDS only, no allocation: capturable as a first call. */
int ddpm_slerp(const float* a, const float* b, const float* alpha, float* out, float* ws, int P, int K, int n, void* stream);
long long ddpm_slerp_workspace_floats(int P, int n);
/* out[r][:] = table[idx[r]][:], fp32 rows of row_len (% 4 == 0) floats; idx outside [0, table_rows) -> the row is NaN.  Sampling only: every
 * ResidualBlock's time bias fc(act(t_emb)) (unet.py:86, with UNet.embed :122-126,207 in front of it) depends on t alone, so the sampler
 * precomputes the [T][sum Cout] table once per weight version and each step gathers its rows instead of running the embedding MLP. */
int ddpm_gather_rows_f32(const float* table, const long long* idx, float* out, int rows, int row_len, int table_rows, void* stream);
/* One training batch out of a data set that lives on the device — what the reference does per image on the host: the dataset's
 * `transforms` (ToTensor + Normalize(0.5, 0.5), RandomHorizontalFlip; ddpm_torch/datasets.py:28-198) and the DataLoader's collate.
 *   out[b] = T(data[index[b]]), out [B][C][H][W] fp32; data [n_images][C][H][W] contiguous, src_dtype 0 = uint8, 1 = fp32 (else status 2).
 * uint8: T(x) = lut[x], lut = the host transform evaluated on the 256 byte values (bit-identical to it by construction); fp32: a copy
 * (lut may be null).  flip != 0 mirrors sample b along W iff the top bit of the library's counter hash of (seed, index[b]) is set
 * (csrc/common.h dropout_word): a pure function of the seed and the DATASET index, not of the position in the batch.
 * An index outside [0, n_images) fills that sample with NaN and touches no other.  C*H*W < 2^31 (else status 1); the data set itself
 * may be any size: image bases are 64-bit offsets from a plain pointer.  No workspace, no atomics. */
int ddpm_batch_gather(const void* data, int src_dtype, const long long* index, const float* lut, float* out,
                      int B, long long n_images, int C, int H, int W, int flip, unsigned long long seed, void* stream);

/* nn.SiLU on the time-embedding path (unet.py:86,124) */
int ddpm_silu_fwd(const float* x, float* y, long long n, void* stream);
int ddpm_silu_bwd(const float* x, const float* dy, float* dx, long long n, int accumulate, void* stream);

/* bias / time-bias gradients: per_sample[b][c] += sum_pixels dy, total[c] += sum_{b,pixels} dy (fp32 atomics into
 * zero-initialised buffers); C <= 64 x 256 16-byte vectors per launch (groups of 256 on blockIdx.z).  No operand limit (64-bit
 * element offsets); B <= 65535 (blockIdx.y). */
int ddpm_colsum(const void* dy, long long ld, float* per_sample, long long ps_ld, float* total, int B, int HW, int C, int dtype, void* stream);
/* backward of nn.Upsample(2,"nearest"): dx[b,y,x,c] (+)= sum of the 2x2 block of dy_up.  No operand limit (64-bit element offsets). */
int ddpm_upsample2x_bwd(const void* dy_up, void* dx, long long dx_ld, int B, int H, int W, int C, int accumulate, int dtype, void* stream);
/* 2x resampling WITHOUT a convolution — UNet(resample_with_conv=False): ddpm_torch/models/unet.py:169 `nn.AvgPool2d(2)`, :196
 * `nn.Upsample(scale_factor=2, mode="nearest")` on its own — and their autograd.  NHWC with pixel pitches; H, W = the SMALL grid.
 *   up = 0: y[b,h,w,:] (+)= scale * (x[b,2h,2w,:] + x[b,2h,2w+1,:] + x[b,2h+1,2w,:] + x[b,2h+1,2w+1,:])   (AvgPool forward: 0.25; Upsample backward: 1)
 *   up = 1: y[b,2h+a,2w+b,:] (+)= scale * x[b,h,w,:], a, b in {0, 1}                                       (Upsample forward: 1; AvgPool backward: 0.25) */
int ddpm_resample2x_nhwc(const void* x, long long x_ld, void* y, long long y_ld, int B, int H, int W, int C, int up, float scale,
                         int accumulate, int dtype, void* stream);
/* y (+)= x over [rows][C] slices with pitches (gradient fan-in of the residual / skip connections).  No operand limit (64-bit
 * element offsets). */
int ddpm_add_rows(const void* x, long long x_ld, void* y, long long y_ld, long long rows, int C, int accumulate, int dtype, void* stream);

/* torch.softmax over the keys (unet.py:47-49) and its backward dS = P*(dP - sum(dP*P)); rows of length L */
int ddpm_softmax_fwd(const float* s, void* p, long long rows, int L, int dtype, void* stream);
int ddpm_softmax_bwd(const void* p, const float* dp, void* ds, long long rows, int L, int dtype, void* stream);

/* nn.utils.clip_grad_norm_ + torch.optim.Adam + EMA.update (ddpm_torch/utils/train.py:159-165,300-305; train.py:128)
 * over one fp32 tensor: total_sq[0] += ||g||^2 (workspace >= 1024 floats); then one fused pass
 *   g' = g * min(1, max_norm/(sqrt(total_sq)+1e-6)); m,v <- Adam moments; p -= lr/bc1 * m/(sqrt(v/bc2)+eps);
 *   shadow += ema_w * (p - shadow)      (total_sq null or max_norm <= 0: no clipping; shadow null: no EMA). */
int ddpm_sumsq_accumulate(const float* g, long long n, float* total_sq, float* workspace, void* stream);
int ddpm_adam_ema_step(float* p, const float* g, float* m, float* v, float* shadow, long long n, const float* total_sq,
                       float max_norm, float lr, float beta1, float beta2, float eps, float bias_corr1, float bias_corr2,
                       float ema_w, void* stream);

/* multi-tensor forms: ONE launch over every parameter tensor.  table[i] = {p, g, m, v, shadow (0 = none), numel} (int64).
 * ddpm_mt_grad_sumsq: total_sq holds ddpm_mt_sumsq_slots(n_tensors) floats; on return total_sq[0] = sum ||g_i||^2 (lanes 1..63 zero),
 * added up in a fixed order (see ddpm_wgrad_unpack_sumsq; total_sq_floats < ddpm_mt_sumsq_slots(n_tensors) -> DDPM_ERR_SHAPE).
 * ddpm_mt_adam_ema: the fused update above for all i, with the clipping norm taken from the sum of the 64-float bank at total_sq — it
 * reads total_sq[0..63] and nothing behind them, so a 64-float buffer is enough for this call. */
int ddpm_mt_sumsq_slots(int n_tensors);
int ddpm_mt_grad_sumsq(const long long* table, int n_tensors, float* total_sq, long long total_sq_floats, void* stream);
/* hyper_dev (optional, 4 device floats {lr, bias_corr1, bias_corr2, ema_w}) overrides the by-value scalars: the values of the
 * current step are read from memory, so one captured hipGraph serves every training step. */
int ddpm_mt_adam_ema(const long long* table, int n_tensors, const float* total_sq, float max_norm, float lr, float beta1,
                     float beta2, float eps, float bias_corr1, float bias_corr2, float ema_w, const float* hyper_dev, void* stream);

/* dst_i = a_i (+ b_i) over many small fp32 tensors in one launch: table[i] = {a, b (0 = none), dst, numel} (int64).  Builds the
 * concatenated time-bias projection (all ResidualBlock.fc weights; fc.bias + conv1.bias, ddpm_torch/models/unet.py:77,85-86). */
int ddpm_mt_gather_f32(const long long* table, int n_tensors, void* stream);

/* ---- the 2-D toy denoiser, BASELINE config 1 (upstream toy/toy_model.py:17-62, csrc/toymlp.hip), fp32 only.
 *   Decoder(D, M, L):  h_0 = x W_in^T (toy_model.py:44,59);  e[t] = enc(lrelu(t_proj(temb(t)))) (:53-55,57-58; TemporalLayer.enc :26,35);
 *   h_{l+1} = h_l + fc2(lrelu(LN2(fc1(lrelu(LN1(h_l))) + e[t])))  with ONE TemporalLayer object used L times (:32-37,47-48,60);
 *   y = out_fc(LN_out(h_L)) + out_fc.b (:49-50,61).  LayerNorm eps 1e-5 (affine), LeakyReLU slope 0.02 (:14), temb as ddpm_timestep_embedding.
 * Geometry: 1 <= D <= 16, M % 32 == 0 with 32 <= M <= 256, L >= 1, B >= 1, 1 <= T <= 4096; anything else DDPM_ERR_SHAPE.  Weights are the
 * module's fp32 tensors (nn.Linear layout [out][in]); fc1_w / fc2_w 16-byte aligned.  t outside [0, T) makes that row NaN.
 *
 * ddpm_toy_time_table (toy_model.py:57-58 + :35 `self.enc(t_emb)`): tabs [2][T][M] = {E[t] = enc(c[t]), c[t] = lrelu(t_proj(temb(t)))} for
 * every t < T, computed from the live parameters on every call (c is the enc input and the LeakyReLU mask of the backward).
 * freqs: the M/2 fp32 frequencies of ddpm_timestep_embedding. */
int ddpm_toy_time_table(const float* freqs, const float* tproj_w, const float* tproj_b, const float* enc_w, const float* enc_b,
                        float* tabs, int T, int M, void* stream);
/* Decoder.forward (toy_model.py:56-62) for x [B][D], t [B] int64, one launch: y [B][D].  saved (null: inference) receives what the
 * backward needs: [L+1][B][M] h_0..h_L, then [B][2L+1][2] (mean, rstd) of LN1 / LN2 of every layer and of LN_out (toy_model.py:33-34,61). */
int ddpm_toy_decoder_fwd(const float* x, const long long* t, const float* w_in, const float* n1_w, const float* n1_b, const float* fc1_w,
                         const float* n2_w, const float* n2_b, const float* fc2_w, const float* on_w, const float* on_b, const float* out_w,
                         const float* out_b, const float* tabs, float* y, float* saved, int B, int D, int M, int L, int T, void* stream);
/* autograd of Decoder.forward (toy_model.py:56-62) except the time path: from dy [B][D] and the forward's saved buffer,
 *   dx [B][D] (null: not wanted);
 *   grads = [in_fc.w M*D][norm1.w M][norm1.b M][fc1.w M*M][norm2.w M][norm2.b M][fc2.w M*M][out_norm.w M][out_norm.b M][out_fc.w D*M][out_fc.b D]
 *           (the shared layer's gradients summed over its L uses);
 *   dzsum [B][M] = sum over layers of the gradient at the fc1 output (= at e[t] of that row; input of ddpm_toy_time_table_bwd).
 * Every output is overwritten.  ws: ws_floats >= 4*r(L*B*M) + r(2*S*M*M) + r(ceil(B/32)*(6M + 2MD + D)) with r(n) = n rounded up to a
 * multiple of 64 and S = min(64, max(1, ceil(L*B/512))) — per-row operands of the weight gradients and per-block partial slabs, summed in
 * a fixed order (no atomics: bit-identical on repetition). */
int ddpm_toy_decoder_bwd(const float* x, const long long* t, const float* dy, const float* w_in, const float* n1_w, const float* n1_b,
                         const float* fc1_w, const float* n2_w, const float* n2_b, const float* fc2_w, const float* on_w, const float* on_b,
                         const float* out_w, const float* tabs, const float* saved, float* dx, float* grads, float* dzsum, float* ws,
                         long long ws_floats, int B, int D, int M, int L, int T, void* stream);
/* autograd of the time table (toy_model.py:57-58, :26,35): dE[t] = sum of dzsum over the rows with that t (row order), then
 * gtab = [enc.w M*M][enc.b M][t_proj.0.w M*M][t_proj.0.b M] (overwritten).  ws: ws_floats >= 3*T*M. */
int ddpm_toy_time_table_bwd(const long long* t, const float* dzsum, const float* freqs, const float* enc_w, const float* tabs, float* gtab,
                            float* ws, long long ws_floats, int B, int M, int T, void* stream);

/* ---- improved precision / recall (csrc/manifold.hip): the two manifold computations without the N x N distance matrix.
 * Operands are fp16, row-major [N][ld] with ld in elements (ld >= D, ld % 8 == 0, 16-byte aligned base), D % 8 == 0, every operand below
 * 2 GiB.  The distance is the one of the block path (widen to fp32, round the result to fp16):
 *   d2(i,j) = max(|r_i|^2 + |c_j|^2 - 2 <r_i, c_j>, 0) in fp32 (fp16 products accumulated in fp32 on the matrix cores),
 *   d(i,j)  = fp16_rne(sqrtf(d2(i,j))), overflow -> inf.
 * Both calls are stream-ordered, allocate nothing and are bit-deterministic (no floating-point atomics).  Scratch is the caller's
 * `workspace` (16-byte aligned, workspace_bytes = its capacity; DDPM_ERR_SHAPE when it is too small).  With
 *   RT = ceil(Nr / 128), CT = ceil(Nc / 128), H = ceil(CT / 2), S0 = min(CT, 64, ceil(4096 / RT)), S1 = min(S0, H) if RT * H >= 512 else S0,
 *   S = ceil(CT / ceil(CT / S1))   (the column split: grid = RT x S workgroups)
 * the radii need 4 * (Nr + Nc) + 64 * S * Nr bytes and the coverage needs 4 * (Np + Ns) bytes.
 * Refused on the host before any launch: null pointer 5; D % 8 != 0, ld < D, N < 1, rank outside [1, min(16, Nc)], an operand of 2 GiB
 * or more, a short workspace 1; a misaligned base or pitch 3.
 *
 * ManifoldBuilder.compute_distance + kthvalue (metrics/precision_recall.py:43-55,156-164):
 *   out[i] (fp16) = the rank-th smallest of d(i, 0 .. Nc-1), rank = nhood_size + 1, equal values counted with multiplicity; a row that
 *   is also a column is an ordinary column (its distance to itself takes part, as upstream). */
int ddpm_manifold_kth_f16(const void* rows, long long rows_ld, int Nr, const void* cols, long long cols_ld, int Nc, int D, int rank,
                          void* out, void* workspace, long long workspace_bytes, void* stream);
/* calc_pr's membership test (metrics/precision_recall.py:188-204):
 *   hit[i] (uint8, 0 or 1) = any_j d(i,j) <= support_kth[j], compared as fp16 values; support_kth is fp16 [Ns]. */
int ddpm_manifold_cover_f16(const void* probe, long long probe_ld, int Np, const void* support, long long support_ld, int Ns, int D,
                            const void* support_kth, void* hit, void* workspace, long long workspace_bytes, void* stream);

/* ---- launch plans (no upstream counterpart: the reference issues its step op by op from Python, ddpm_torch/utils/train.py:148-170).
 * The training step is a fixed sequence of the calls above; a plan records it once — entry-point name + argument words + the
 * hipStream_t each call was given — and ddpm_plan_run re-issues a whole segment from C: eager semantics (two concurrent streams,
 * host work such as RCCL calls between segments) without the interpreter between launches.  Step-varying scalars must live in
 * device memory (hyper_dev, seed_dev), exactly as for a captured hipGraph; every pointer recorded must stay valid while the plan lives.
 *
 * ddpm_stream_order(waiter, signaller): everything enqueued on hipStream_t `waiter` after the call runs after everything enqueued on
 * `signaller` before it (event record + stream wait on a pooled event) — the fork / join edges of the weight-gradient stream.
 * ddpm_fill_zero: stream-ordered memset(0) (torch.zeros / Tensor.zero_ of the gradient staging buffers).
 * ddpm_plan_append: words[i] = argument i of `entry` as a 64-bit word (pointers / 64-bit integers as they are, int in the low half,
 * float as its IEEE-754 bits in the low half); returns the entry index or -(status) (unknown name or wrong argument count: -1).
 * ddpm_plan_cut closes the current segment (returns its index).  ddpm_plan_run issues segment `segment` and returns 0 or the status of
 * the first failing call (ddpm_plan_failed_entry names it).  A plan is not thread-safe; distinct plans are independent. */
int ddpm_stream_order(void* waiter, void* signaller);
int ddpm_fill_zero(void* p, long long bytes, void* stream);
void* ddpm_plan_create(void);
int ddpm_plan_destroy(void* plan);
int ddpm_plan_append(void* plan, const char* entry, const unsigned long long* words, int n_words);
int ddpm_plan_cut(void* plan);
int ddpm_plan_segments(void* plan);
int ddpm_plan_entries(void* plan);
int ddpm_plan_run(void* plan, int segment);
const char* ddpm_plan_failed_entry(void* plan, int* index);
int ddpm_plan_entry_arity(const char* entry);

#ifdef __cplusplus
}
#endif
#endif
