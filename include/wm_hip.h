/* wm_hip.h -- C ABI of libwm_hip.so: the MI355X (gfx950) kernels of the watermark embed+detect hot path.
 *
 * The reference (py/main16.py) has no FFI: its boundary for this path is the nn.Module call
 *   Generator.forward(s, message)  py/main16.py:149-162
 *   Detector.forward(x)            py/main16.py:183-186
 * plus the free functions / loss modules of py/main16.py:53-81 and :192-217.  Everything those calls reach in
 * ATen (conv1d, batch_norm, lstm, conv_transpose1d, embedding, stft, ...) is replaced by the stateless launchers
 * below; the host-side mirror of the nn.Module API lives in the Python package and binds this file with ctypes
 * (see INTEGRATION.md for the binding a maintainer of the reference would add).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 unless stated (message: int64, tables: int32);
 *   - activations are channel-first frames [B,64,T] exactly as the reference holds them, T % 4 == 0;
 *   - inputs are borrowed and never written; outputs / scratch are caller-allocated;
 *   - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream); launchers enqueue and return,
 *     they never synchronise, allocate or free (graph-capture safe).  State kept across calls: (a) a per-device
 *     cache of "dynamic-LDS opt-in done" bits (hipFuncSetAttribute is per device; idempotent, so launchers are
 *     safe from several host threads and for one process driving several GPUs); (b) the two PROCESS-WIDE
 *     experiment knobs wm_set_conv_bf_schedule / wm_set_lstm_dx_bf16x6 below -- they select between kernel
 *     generations of equal results, are meant to be set once at start-up (or never: the defaults are the fast
 *     builds) and are not synchronised with launches issued concurrently from other threads;
 *   - return value: 0 on success, else a hipError_t value (1 = invalid argument / unsupported variant).
 */
#ifndef WM_HIP_H
#define WM_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* wm_stream_t;   /* == hipStream_t */

/* ---- 64->64 convolutions on the fp32 matrix cores -------------------------------------------------------------
 * replace nn.Conv1d(64,64,3,padding=1) of ResBlock (py/main16.py:116,119) and nn.ConvTranspose1d(64,64,7,padding=3)
 * (py/main16.py:144), forward and backward.                                                                     */

/* w -> GEMM image wp[KW][64 in][64 out].  mode 0 Conv1d fwd | 1 Conv1d dgrad | 2 ConvTranspose1d fwd | 3 ConvT dgrad */
int wm_pack_w64(const float* w, float* wp, int KW, int mode, wm_stream_t stream);

/* y = conv_same(pro(x)) then epi.
 *   pro: 0 x | 1 relu(x*pa[c]+pb[c]) (BatchNorm+ReLU folded into the load, py/main16.py:117-118)
 *        | 2 x + pa[b*64+c] (message embedding add, py/main16.py:158-159) | 3 pa[c]*x + (pb[c] + pb[64+c]) + pc[c]*x2 (BN backward; pb is [2][64]: offset as hi + lo words)
 *   epi: 0 + bias[c] | 1 keep where e1*ea[c]+eb[c] > 0 (ReLU backward) | 2 + e1 (residual gradient) | 3 none
 *   stats (NULL or [256][2][64]): per-workgroup partial sums for BatchNorm (epi 0: sum y, sum y^2;
 *   epi 1: sum v, sum v*e1); all 256 slots are written or zeroed.  Supported (KW,pro,epi): (3,{0,1},0) with or without stats,
 *   (3,3,1) with stats only, (3,3,{2,3}) without; (7,{0,2},0) and (7,0,3) without stats.  Anything else: hipErrorInvalidValue. */
int wm_conv64(const float* x, const float* x2, const float* wp, const float* pa, const float* pb, const float* pc,
              const float* bias, const float* e1, const float* ea, const float* eb, float* y, float* stats,
              int B, int T, int KW, int pro, int epi, wm_stream_t stream);

/* bf16x6 build of the k3 convolution: every fp32 operand is split into three bf16 pieces in LDS and the six piece
 * products of weight >= 2^-16 are accumulated in fp32 on the bf16 matrix cores (fp32-grade error, 6/16 of the fp32 MFMA
 * time).  Same pro / epi / stats contract as wm_conv64 with KW = 3; wpb [3][3][64][64] uint16 from wm_pack_w64_bf
 * (mode 0 Conv1d fwd | 1 Conv1d dgrad).  One more epilogue exists here only, for inference (py/main16.py:124-125 in
 * eval mode as two launches): (pro 1, epi 4, stats NULL) y = relu(e1 + (conv + bias[c]) * ea[c] + eb[c]), i.e. the
 * second conv of a ResBlock with BatchNorm2 (folded running statistics), the residual add and the ReLU in its epilogue;
 * needs schedule 2 and T % 128 == 0 (hipErrorInvalidValue otherwise).
 * For the 64-channel stride-1 blocks of the main14b_2 variant (py/main14b_2.py:95-102, no BatchNorm; pro 0, stats NULL, any
 * T % 4 == 0, phase-serial kernel): epi 5 y = elu(conv + bias) | 6 y = elu(conv + bias + e1) | 7 y = conv * ELU'(e1), e1 = the ELU
 * output the gradient flows into | 2 y = conv + e1 | 3 y = conv. */
int wm_pack_w64_bf(const float* w, void* wpb, int mode, wm_stream_t stream);
/* schedule of wm_conv64_bf (process-wide knob; default 2): 0 phase-serial, one wave per SIMD, 128-column tiles |
 * 2 weight fragments resident in registers, input image double-buffered, split / deferred epilogue / prefetch dealt out one
 * slice per MFMA (T % 128 == 0, else 0 runs).  Any other value selects 0. */
int wm_set_conv_bf_schedule(int schedule, wm_stream_t stream);
int wm_conv64_bf(const float* x, const float* x2, const void* wpb, const float* pa, const float* pb, const float* pc,
                 const float* bias, const float* e1, const float* ea, const float* eb, float* y, float* stats,
                 int B, int T, int pro, int epi, int arith, wm_stream_t stream);
/* arith 0: bf16x6, wpb from wm_pack_w64_bf.  arith 1: f16 two-piece split, three products per product on v_mfma_f32_32x32x16_f16
 * (see wm_dwgrad64_bf below), wpb from wm_pack_w64_h(mode 0); only (pro 0 | 1, epi 0, with or without stats) and (pro 1, epi 4) under
 * schedule 2 with T % 128 == 0 -- the ResBlock forward convolutions -- hipErrorInvalidValue otherwise.  Activations are split unscaled: the
 * representation floor is 2^-25 ABSOLUTE (f16 subnormal spacing / 2) on top of 2^-22 relative, i.e. fp32-grade for the O(1)
 * activations BatchNorm + ReLU produce. */
/* conv1 of a training ResBlock whose input is the tail of the block in front of it, formed while the tile is staged instead of by a
 * wm_bn_add_relu_mask launch of its own: out = relu(x + y2 * sc2 + sh2) and its sign bits (mask: wm_bn_add_relu_mask's layout, may be
 * NULL) are written as side products, bit for bit what that launch writes; y and stats are bit for bit wm_conv64_bf(pro 0, epi 0,
 * arith 1) on that out.  wpb_h from wm_pack_w64_h(mode 0); stats is required.  The pipelined f16 build only: T % 128 != 0 or
 * schedule 0 is hipErrorInvalidValue, and nothing is written. */
int wm_conv64_bf_tail(const float* x, const float* y2, const void* wpb_h, const float* sc2, const float* sh2, const float* bias,
                      float* out, void* mask, float* y, float* stats, int B, int T, wm_stream_t stream);

/* The first training ResBlock's conv1 with the stem Conv1d(1, 64, 7, padding = 3) formed on load (py/main16.py:134-135, :177-178)
 * instead of a wm_stem_fwd launch of its own: the clips s [B,1,T] are read in place of a frame, y0 [B,64,T] = the stem's output is
 * written as a side product, bit for bit what wm_stem_fwd(s, stem_w, stem_b) writes; y and stats are bit for bit wm_conv64_bf(pro 0,
 * epi 0, arith 1) on that y0.  stem_w [64,7], stem_b [64]; wpb_h from wm_pack_w64_h(mode 0); stats is required.  The pipelined f16
 * build only: T % 128 != 0, schedule 0 or a null pointer is hipErrorInvalidValue, and nothing is written. */
int wm_conv64_bf_stem(const float* s, const float* stem_w, const float* stem_b, const void* wpb_h, const float* bias, float* y0,
                      float* y, float* stats, int B, int T, wm_stream_t stream);

/* Inference ResBlock as ONE launch (py/main16.py:112-125 with both BatchNorm1d in eval mode):
 *   y = relu(x + (conv2(relu((conv1(x) + b1) * sc1 + sh1)) + b2) * sc2 + sh2)
 * sc / sh = the folded running statistics (wm_bn_eval_scale_shift); w1pb / w2pb = wm_pack_w64_bf_scaled images of
 * w1 * sc1[out] / w2 * sc2[out] (the per-channel scale rides in the weights, the kernel adds b * sc + sh); b1 / b2 may be NULL.
 * Two frame passes over HBM (x in, y out): the intermediate activation stays in LDS as bf16x3 pieces.  T % 4 == 0. */
int wm_pack_w64_bf_scaled(const float* w, const float* row_scale, void* wpb, wm_stream_t stream);
int wm_resblock_eval_bf(const float* x, const void* w1pb, const void* w2pb, const float* b1, const float* sc1, const float* sh1,
                        const float* b2, const float* sc2, const float* sh2, float* y, int B, int T, int arith, wm_stream_t stream);
/* arith 0: bf16x6 (images from wm_pack_w64_bf_scaled).  arith 1: f16 two-piece split, three products per product; images from
 * wm_pack_w64_h_scaled (w * sc[out] * ws, {ws, 1 / ws} behind the image), x and the intermediate split unscaled. */
int wm_pack_w64_h_scaled(const float* w, const float* row_scale, void* wph, wm_stream_t stream);

/* Data gradient AND weight gradient of a 64->64 k3 convolution in ONE launch (ResBlock backward, py/main16.py:112-125 under
 * autograd): g = ga[c] dz + gb[c] + gb[64+c] + gc[c] y is rebuilt once and feeds both; frames moved: 4 (conv2 pair) / 5 (conv1
 * pair) instead of 7.  wpb = wm_pack_w64_bf mode-1 image.  Two forms:
 *   xpro 1, epi 1: x' = relu(x xa + xb) is the weight gradient's input operand; y = data gradient masked by (e1 ea + eb > 0),
 *                  stats [256][2][64] = (sum y, sum y e1) per workgroup (reduce with wm_bn_bwd_finalize)       [conv2 of a block]
 *   xpro 0, epi 2: x as is; y = data gradient + e1; stats NULL                                                 [conv1 of a block]
 *   xpro 0, epi 8: the second form for a block that FOLLOWS another ResBlock: y = (data gradient + e1) masked by the sign bits of
 *                  the previous block's output (eb = that mask, passed as const float*), stats = (sum y, sum y ea) with ea = the
 *                  previous block's pre-BatchNorm activation y2 [B,64,T]: the previous block's ReLU backward and BatchNorm sums
 *                  ride in this launch's epilogue (it then needs neither wm_relu_bwd_reduce_mask nor a mask of its own); needs gmask.
 * gmask (optional): the sign bits wm_bn_add_relu_mask wrote for the block output.  With it the gradient that reaches the block
 * output is passed as it arrived and masked on load -- as dz in the first form, as e1 in the second -- so the masked copy
 * dz = g (out > 0) never exists in memory (wm_relu_bwd_reduce_mask with dz = NULL supplies the two BatchNorm sums).
 * dw [out][in][3] / dbias [64] as wm_wgrad64_bf (partial: 256 x (3*4096+64) floats of scratch; accumulate 0 | 1).  T % 64 == 0. */
int wm_dwgrad64_bf(const float* g, const float* g2, const float* ga, const float* gb, const float* gc, const void* wpb,
                   const float* x, const float* xa, const float* xb, const float* e1, const float* ea, const float* eb,
                   float* y, float* stats, float* partial, float* dw, float* dbias, int B, int T, int xpro, int epi, int accumulate,
                   const void* gmask, int arith, const float* gscale, float* dzmax, wm_stream_t stream);
/* arith 0: bf16 three-piece split, six piece products (bf16x6); wpb from wm_pack_w64_bf.
 * arith 1: f16 TWO-piece split (22 bits per operand), three products on v_mfma_f32_32x32x16_f16 -- half the matrix work of arith 0,
 *          wpb from wm_pack_w64_h (weights scaled by a
 *          power of two chosen from max |w|, stored behind the image); gscale = wm_bn_bwd_finalize's {gs, 1 / gs} for THIS launch's
 *          g; dzmax (optional, epi 1 / 2 / 8; arith 1 only, arith 0 leaves it untouched): 256 floats, max |y| per workgroup (slots
 *          beyond the grid zeroed) = the dzmax input of the next launch's finalize. */
int wm_pack_w64_h(const float* w, void* wph, int mode, wm_stream_t stream);      /* 2 * 3 * 4096 f16 + 2 floats */
/* wm_dwgrad64_bf for the ResBlock in front of the Conv1d(64,1,1) head.  The gradient that reaches its output is the rank-one frame
 * hw[c] g1[b][t] (wm_head1_bwd's dx); it is formed on load from g1 [B][T] and hw [64] -- the same single multiply -- and never read
 * from memory.  Two forms only, both with gmask and arith 1: (xpro 1, epi 1) with g == NULL: the frame is the gradient operand;
 * (xpro 0, epi 2) with e1 == NULL: the frame is the epilogue addend.  Anything else: hipErrorInvalidValue.  Every output bit for bit
 * what wm_dwgrad64_bf gives on the materialised frame. */
int wm_dwgrad64_bf_r1(const float* g, const float* g2, const float* ga, const float* gb, const float* gc, const void* wpb,
                      const float* x, const float* xa, const float* xb, const float* e1, const float* ea, const float* eb,
                      float* y, float* stats, float* partial, float* dw, float* dbias, int B, int T, int xpro, int epi, int accumulate,
                      const void* gmask, int arith, const float* gscale, float* dzmax, const float* g1, const float* hw,
                      wm_stream_t stream);
/* wm_dwgrad64_bf's plain conv1 pair (xpro 0, epi 2, no gmask, arith 1) for the first ResBlock behind a stem.  Its weight-gradient
 * operand x is the stem's output Conv1d(1, 64, 7, padding = 3)(s); it is formed on load from the clips s [B,1,T] and stem_w [64,7],
 * stem_b [64] -- wm_stem_fwd's own fmaf chain -- and never read from memory.  e1 = the addend of the data gradient; the other
 * arguments as wm_dwgrad64_bf's of the same names.  A null pointer (dbias and dzmax may be null) or T % 64 != 0:
 * hipErrorInvalidValue, nothing is written.  Every output bit for bit what wm_dwgrad64_bf gives on the materialised x. */
int wm_dwgrad64_bf_stem(const float* g, const float* g2, const float* ga, const float* gb, const float* gc, const void* wpb,
                        const float* e1, float* y, float* partial, float* dw, float* dbias, int B, int T, int accumulate,
                        const float* gscale, float* dzmax, const float* s, const float* stem_w, const float* stem_b,
                        wm_stream_t stream);

/* bf16x6 build of the 7-tap ConvTranspose1d(64,64,7,padding=3) (py/main16.py:144): wpb [3][7][64][64] uint16 from
 * wm_pack_w64_bf7 (mode 2 forward | 3 data gradient).  pro 0 x | 2 x + vec[b*64+c]; epi 0 + bias[c] | 3 none. */
int wm_pack_w64_bf7(const float* w, void* wpb, int mode, wm_stream_t stream);
int wm_conv64_bf7(const float* x, const void* wpb, const float* vec, const float* bias, float* y, int B, int T, int pro, int epi,
                  int arith, const float* gscale, wm_stream_t stream);
/* arith 0: bf16x6, wpb from wm_pack_w64_bf7.  arith 1 (T % 128 == 0): f16 two-piece split, three products per product, wpb
 * [2][7][64][64] f16 + {ws, 1 / ws} from wm_pack_w64_h7 (same modes); gscale (optional; the data-gradient launch passes it) = {gs, 1 / gs}
 * from wm_gscale_absmax: the input is multiplied by gs before the split and clamped to +-6e4, the result leaves times 1 / (ws gs). */
int wm_pack_w64_h7(const float* w, void* wph, int mode, wm_stream_t stream);     /* 2 * 7 * 4096 f16 + 2 floats */
/* {gs, 1 / gs} for a gradient tensor x [n] (n % 4 == 0): gs = the power of two that puts max |x| into (2^(L-1), 2^L], L = log2_target
 * (12 leaves 2^4 of headroom below the f16 maximum); all-zero / non-finite input gives gs = 1.  scratch >= 1024 floats. */
int wm_gscale_absmax(const float* x, long long n, float* scratch, float log2_target, float* gscale, wm_stream_t stream);
/* the same from per-workgroup maxima a producer already wrote (wm_dwgrad64_bf's dzmax, epi 1 / 2 / 8): no pass over the tensor */
int wm_gscale_from_max(const float* maxes, int n, float log2_target, float* gscale, wm_stream_t stream);
/* out[r] = max |x[r][:]| for x [rows][row_len] (row_len % 4 == 0; out zeroed by the caller, atomic max): the per-clip input maxima of
 * wm_gconv_h (per_clip = 1) for an activation whose producer left none */
int wm_absmax_rows(const float* x, int rows, long long row_len, float* out, wm_stream_t stream);

/* weight gradient of that ConvTranspose1d (= wm_wgrad64 with KW 7, gpro 0, layout 1): dw [in][out][7], dbias [64];
 * xpro 0 | 2 (x + vec[b*64+c]); partial: >= 256 * (7*4096 + 64) floats; accumulate: 0 overwrite | non-zero add (the whole value,
 * not bit 0 alone as in wm_wgrad64_bf: there is no output-split build here). */
int wm_wgrad64_bf7(const float* g, const float* x, const float* vec, float* partial, float* dw, float* dbias, int B, int T,
                   int xpro, int accumulate, int arith, const float* gscale, wm_stream_t stream);
/* arith 1: f16 two-piece split; gscale = wm_gscale_absmax's {gs, 1 / gs} for g (required), x is split unscaled, dbias from the unscaled g */

/* bf16x6 build of the k3 Conv1d weight gradient (contract of wm_wgrad64 with KW = 3, layout 0; gpro / xpro (3,1), (3,0), (0,0); partial:
 * 256 x (3*4096+64) floats).  accumulate: bit 0 = add to
 * dw / dbias, bit 1 = the output-split build (a wave keeps one 32x32 block per tap: ~200 registers per lane, so the workgroup
 * can share a CU with the LSTM recurrence kernels when it is launched on a side stream; same results; (0,0) has no such build and
 * ignores the bit)                                                                                                          */
int wm_wgrad64_bf(const float* g, const float* g2, const float* ga, const float* gb, const float* gc,
                  const float* x, const float* xa, const float* xb, float* partial, float* dw, float* dbias,
                  int B, int T, int gpro, int xpro, int accumulate, wm_stream_t stream);

/* dW (+)= sum_{b,t} gpro(g)[out,t] * xpro(x)[in,t+tap-KW/2]; dbias (+)= sum gpro(g).  partial: [256][KW*4096+64] (one slab per
 *   workgroup, at most 256).  Supported (KW,gpro,xpro): (3,3,1) (3,3,0) (7,0,2) (7,0,0), anything else hipErrorInvalidValue; prologues
 *   as above; layout 0: Conv1d weight [out][in][KW], 1: ConvTranspose1d weight [in][out][KW] (either with either KW); accumulate:
 *   0 overwrite | non-zero add. */
int wm_wgrad64(const float* g, const float* g2, const float* ga, const float* gb, const float* gc,
               const float* x, const float* xa, const float* xb, float* partial, float* dw, float* dbias,
               int B, int T, int KW, int gpro, int xpro, int layout, int accumulate, wm_stream_t stream);

/* ---- BatchNorm1d(64) glue (py/main16.py:117,120) ----------------------------------------------------------- */
int wm_bn_finalize(const float* partials, int nparts, double count, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, long long* num_batches_tracked, float momentum, float eps,
                   float* scale, float* shift, float* save_mean, float* save_invstd, wm_stream_t stream);
int wm_bn_eval_scale_shift(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                           float eps, float* scale, float* shift, wm_stream_t stream);
/* ResBlock tail  out = relu(x + y2*scale + shift)  (py/main16.py:125) and its backward + BN-backward reductions */
int wm_bn_add_relu(const float* x, const float* y2, const float* scale, const float* shift, float* out, int B, int T,
                   wm_stream_t stream);
int wm_relu_bwd_reduce(const float* g, const float* out, const float* y2, float* dz, float* partial, int B, int T,
                       wm_stream_t stream);
/* The same pair with the sign of `out` carried as one bit per element: mask = ceil(T / 32) 32-bit words per (clip, channel) row,
 * B * 64 rows, bit (t % 32) of word t / 32 set where out > 0.  The backward then reads g, y2 and 3 % of a frame instead of g, out,
 * y2; with dz = NULL it only forms the two sums (the masked gradient is then rebuilt on load by wm_dwgrad64_bf's gmask).  What
 * ResBlock training uses. */
int wm_bn_add_relu_mask(const float* x, const float* y2, const float* scale, const float* shift, float* out, void* mask, int B, int T,
                        wm_stream_t stream);
int wm_relu_bwd_reduce_mask(const float* g, const void* mask, const float* y2, float* dz, float* partial, float* dzmax, int B, int T,
                            wm_stream_t stream);      /* dzmax (optional): B * 64 floats, max |dz| per row (wm_bn_bwd_finalize's gscale) */
/* wm_relu_bwd_reduce_mask(dz = NULL) on the rank-one frame g[b][c][t] = w[c] g1[b][t] (wm_head1_bwd's dx), formed on load from
 * g1 [B][T] and w [64]: partial and dzmax bit for bit the same. */
int wm_relu_bwd_reduce_mask_r1(const float* g1, const float* w, const void* mask, const float* y2, float* partial, float* dzmax, int B,
                               int T, wm_stream_t stream);
/* A, Cc: [64]; Bc: [2][64] (hi, lo words of the offset, see wm_conv64 pro 3) */
int wm_bn_bwd_finalize(const float* partials, int nparts, double count, const float* gamma, const float* save_mean,
                       const float* save_invstd, float* A, float* Bc, float* Cc, float* dgamma, float* dbeta,
                       int accumulate, int eval_mode, const float* dzmax, int nmax, float* gscale, wm_stream_t stream);
/* gscale (optional, 2 floats; needs dzmax [nmax] = max |dz| per producer block): {gs, 1 / gs}, gs = the power of two that brings
 * max |A| * max |dz| to 2^9 -- the scale under which wm_dwgrad64_bf (arith 1) splits the rebuilt gradient into two f16 pieces. */

/* ---- stem / heads: Conv1d(1,64,7,p=3) :134,:177 ; Conv1d(64,1,1) :146 ; Conv1d(64,1+bits,1) :180 (+permute :186) */
int wm_stem_fwd(const float* s, const float* w, const float* bias, float* y, int B, int T, wm_stream_t stream);
int wm_stem_bwd(const float* g, const float* s, const float* w, float* ds, float* partial, float* dw, float* db, int B,
                int T, int nds, int accumulate, wm_stream_t stream);   /* ds rows only for clips [0, nds); partial >= 512*512 floats */
int wm_head1_fwd(const float* x, const float* w, const float* bias, float* y, int B, int T, wm_stream_t stream);
int wm_head1_bwd(const float* g, const float* x, const float* w, float* dx, float* partial, float* dw, float* db, int B,
                 int T, int accumulate, wm_stream_t stream);   /* dx == NULL: dw and db only (the _r1 entry points rebuild dx on load) */
/* logits written as (B,T,NO) contiguous -- the layout Detector.forward's permuted view exposes.  NO = 1 + message_bits,
 * 1 <= NO <= 64 (message ids are int64, so at most 63 bits); T % 4 == 0.  headN_bwd: partial >= 256*(NO*64+NO) floats. */
int wm_headN_fwd(const float* x, const float* w, const float* bias, float* y, int B, int T, int NO, wm_stream_t stream);
int wm_headN_bwd(const float* g, const float* x, const float* w, float* dx, float* partial, float* dw, float* db, int B,
                 int T, int NO, int accumulate, wm_stream_t stream);
/* The heads with the ResBlock tail in front of them (the last block of each net, py/main16.py:145-146, :179-180): the kernel forms
 * out = relu(x + y2*scale + shift) itself -- wm_bn_add_relu's expression, so `out` is bit-identical -- stores it once (it is the saved
 * input of the head's backward and nothing else) and never reads it back; y / logits are bit-identical to wm_head1_fwd(out) /
 * wm_headN_fwd(out).  mask (optional): the sign bits of `out` in wm_bn_add_relu_mask's layout, bits at t >= T zero; NULL = none
 * (no gradient wanted).  x, y2, out: [R,64,T]; scale, shift: [64].  wm_head1_tail_fwd needs y2 and T % 4 == 0.
 * wm_headN_tail_fwd: y2 == NULL = no tail (v = x, `out` and `mask` unused): the plain head, for what follows.
 *   message != NULL ([B] int64, rows [0, B) of the R are the watermarked ones): also both BCE terms of wm_bce_fwd, summed from the
 *   logits while they are in registers -- one fp32 sum pair per workgroup into partial (>= 2 * R * ceil(T / 256) floats), finished in
 *   fp64 and a fixed order with wm_bce_fwd's scales (no atomics: bit-reproducible; against wm_bce_fwd on the same logits the two sums
 *   differ by fp32 rounding, the grouping is another).  NO == 1 leaves bce_out untouched, as wm_bce_fwd does. */
int wm_head1_tail_fwd(const float* x, const float* y2, const float* scale, const float* shift, const float* w, const float* bias,
                      float* out, void* mask, float* y, int B, int T, wm_stream_t stream);
int wm_headN_tail_fwd(const float* x, const float* y2, const float* scale, const float* shift, const float* w, const float* bias,
                      const long long* message, int B, float* partial, float* loc_out, float* bce_out, float* out, void* mask,
                      float* logits, int R, int T, int NO, wm_stream_t stream);
/* wm_bce_bwd + wm_headN_bwd in one launch: in place of g it takes the logits [R,T,NO], message [B] and the device scalars g_loc,
 * g_bce, and forms d(g_loc*loc + g_bce*bce)/d(logits) while it stages the logits -- wm_bce_bwd's expressions, so dx, dw, db are
 * bit-identical to the pair -- and the [R,T,NO] gradient tensor is never written.  partial, accumulate: as wm_headN_bwd. */
int wm_headN_bwd_bce(const float* logits, const long long* message, const float* g_loc, const float* g_bce, const float* x,
                     const float* w, float* dx, float* partial, float* dw, float* db, int B, int R, int T, int NO, int accumulate,
                     wm_stream_t stream);

/* ---- nn.LSTM(64,64,batch_first=True) :138,:152-154 ----------------------------------------------------------
 * csrc/lstm_fwd.hip:  wm_lstm_xproj, wm_lstm_fwd, wm_lstm_fwd_fused, wm_lstm_fwd_tail, wm_set_lstm_fwd_wave_specialised
 * csrc/lstm_bwd.hip:  wm_lstm_bwd, wm_lstm_bwd_fused, wm_lstm_bwd_wgrad, wm_lstm_bwd_wgrad_dx
 * csrc/lstm_grad.hip: wm_lstm_dx, wm_lstm_wgrad, wm_set_lstm_dx_bf16x6 */
int wm_lstm_xproj(const float* x, const float* w_ih, const float* b_ih, const float* b_hh, float* xp, int B, int T,
                  wm_stream_t stream);
int wm_lstm_fwd(const float* xp, const float* w_hh, float* hout, float* gates, float* cst, int B, int T, wm_stream_t stream);
/* xproj + recurrence in one launch: the projection of the next 32 steps runs on the bf16 matrix cores (bf16x6 split,
 * fp32-grade) beside the recurrence and never touches HBM.  gates [B,T,256] / cst [B,T,64] (both or neither): saved
 * activations / cell states for wm_lstm_bwd, exactly as wm_lstm_fwd writes them.  T >= 8. */
int wm_lstm_fwd_fused(const float* x, const float* w_ih, const float* b_ih, const float* b_hh, const float* w_hh,
                      float* hout, float* gates, float* cst, int B, int T, wm_stream_t stream);
/* build of wm_lstm_fwd_fused (process-wide; default 1): 1 wave-specialised -- the recurrence on waves 0..3, the projection of the next
 * 32-step chunk on four helper waves that share its one barrier per step; 0 the projection inside the recurrence's own waves.
 * Bit-identical results. */
int wm_set_lstm_fwd_wave_specialised(int on, wm_stream_t stream);
/* wm_lstm_fwd_fused (always the wave-specialised build) on out = relu(xres + y2 * sc2 + sh2), the tail of the ResBlock in front of the
 * LSTM: the helper waves form it while they stage each 32-step chunk and store `out` and its sign bits (mask: wm_bn_add_relu_mask's
 * layout, may be NULL) bit for bit as that launch writes them; hout / gates / cst are bit for bit wm_lstm_fwd_fused on that out.
 * T % 32 != 0 is hipErrorInvalidValue, and nothing is written: the caller keeps the two launches. */
int wm_lstm_fwd_tail(const float* xres, const float* y2, const float* sc2, const float* sh2, float* out, void* mask, const float* w_ih,
                     const float* b_ih, const float* b_hh, const float* w_hh, float* hout, float* gates, float* cst, int B, int T,
                     wm_stream_t stream);
int wm_lstm_bwd(float* gates, const float* cst, const float* dh_out, const float* w_hh, int B, int T, wm_stream_t stream);
int wm_lstm_dx(const float* da, const float* w_ih, float* dx, int B, int T, wm_stream_t stream);
/* arithmetic of wm_lstm_dx and wm_lstm_wgrad (process-wide): 1 bf16x6 split on the bf16 matrix cores (default,
 * fp32-grade) | 0 native fp32 MFMA */
int wm_set_lstm_dx_bf16x6(int on, wm_stream_t stream);
/* wm_lstm_bwd + wm_lstm_dx in one launch: dx = da W_ih is formed chunk by chunk on the bf16 matrix cores (bf16x6 split)
 * beside the recurrence, from LDS -- no second pass over the [B,T,256] da tensor.  gates: activations in, da out. */
int wm_lstm_bwd_fused(float* gates, const float* cst, const float* dh_out, const float* w_hh, const float* w_ih, float* dx,
                      int B, int T, wm_stream_t stream);
int wm_lstm_wgrad(const float* da, const float* x, const float* h, float* partial, float* dw_ih, float* dw_hh,
                  float* db_ih, float* db_hh, int B, int T, int accumulate, wm_stream_t stream);
/* wm_lstm_bwd + wm_lstm_wgrad in one launch (py/main16.py:141,153 under autograd): four more waves per workgroup form the clip's
 * dW_ih / dW_hh on the matrix cores (bf16x6) out of the 32-step chunk of da the recurrence has just finished, from an LDS image --
 * da is not read back from HBM for them; bias gradients from the recurrence lanes.  gates: saved activations in, da out (still
 * written: wm_lstm_dx reads it).  partial >= B * (256*128 + 256) floats (one slab per clip, reduced in fixed order); accumulate as
 * wm_lstm_wgrad.  T % 32 == 0 and T >= 64 (hipErrorInvalidValue otherwise: use the two separate entry points). */
int wm_lstm_bwd_wgrad(float* gates, const float* cst, const float* dh_out, const float* w_hh, const float* x, const float* h,
                      float* partial, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, int B, int T, int accumulate,
                      wm_stream_t stream);
/* wm_lstm_bwd_wgrad + wm_lstm_dx in one launch: two of the helper waves also form dx = W_ih^T da from the LDS image of the finished
 * chunk, bit for bit wm_lstm_dx's bf16x6 result.  da is never written: gates is read only and keeps the saved activations.  Same
 * conditions as wm_lstm_bwd_wgrad (B > 0, T % 32 == 0, T >= 64); a NULL dx or w_ih, or a partial that is not 16-byte aligned (each
 * clip's slab carries a packed piece of W_ih until its own values replace it), is hipErrorInvalidValue as well, and nothing is
 * written.  After wm_set_lstm_dx_bf16x6(0) the entry point runs the two launches instead, and gates then holds da. */
int wm_lstm_bwd_wgrad_dx(const float* gates, const float* cst, const float* dh_out, const float* w_hh, const float* w_ih,
                         const float* x, const float* h, float* partial, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh,
                         float* dx, int B, int T, int accumulate, wm_stream_t stream);

/* ---- nn.Embedding(2**bits,64) lookup :158 and its dense gradient ------------------------------------------- */
int wm_embed_gather(const float* table, const long long* message, float* vec, int B, int nrows, int* err, wm_stream_t stream);
int wm_embed_scatter_add(float* dtable, const long long* message, const float* dvec, int B, int nrows, wm_stream_t stream);
int wm_rowsum(const float* x, float* out, int rows, int T, wm_stream_t stream);

/* ---- delta post-processing: fir_lowpass :53-64 (bit 0), clamp_peak :66-67 (bit 1), limit_rms :69-72 (bit 2) -- */
int wm_postproc_fwd(const float* d_in, const float* taps, int ntaps, float thr, float max_rms, float eps, int stages,
                    float* f_out, float* d_out, float* stats, int B, int T, wm_stream_t stream);
int wm_postproc_bwd(const float* g, const float* f_in, const float* stats, const float* taps, int ntaps, float thr,
                    float max_rms, int stages, float* d_raw, int B, int T, wm_stream_t stream);

/* ---- STFT loss stack: MultiScaleMelLoss :192-202, TFLoudnessLoss :204-217, high_freq_penalty :74-81 ---------
 * loss_out: device scalar.  dsig (NULL = forward only): d loss / d (second signal | delta), [B,T].
 * gframes: scratch [B, 1+T/hop, n_fft]; partial: scratch [B*(1+T/hop)].                                          */
int wm_mel_loss(const float* clean, const float* wm, const float* fb, const int* klo, const int* khi, const int* mlo,
                float* gframes, float* partial, float* loss_out, float* dsig, int B, int T, wm_stream_t stream);
int wm_loud_loss(const float* clean, const float* wm, float thresh, float* gframes, float* partial, float* loss_out,
                 float* dsig, int B, int T, wm_stream_t stream);
int wm_hf_penalty(const float* delta, int kcut, float* gframes, float* partial, float* loss_out, float* dsig, int B, int T,
                  wm_stream_t stream);

/* ---- point-wise losses :252-266 and the optimizer update :504,:278 ------------------------------------------
 * wm_bce_*: logits [R = 2B][T][NO]; partial: >= 2 * R * ceil(T*NO / 4096) floats of scratch; T*NO < 2^23, R <= 65535 */
int wm_bce_fwd(const float* logits, const long long* message, float* partial, float* loc_out, float* bce_out, int B, int R,
               int T, int NO, wm_stream_t stream);
int wm_bce_bwd(const float* logits, const long long* message, const float* g_loc, const float* g_bce, float* dlogits, int B,
               int R, int T, int NO, wm_stream_t stream);
int wm_l1_fwd(const float* x, float* partial, float* out, long long n, wm_stream_t stream);
int wm_l1_bwd(const float* x, const float* g, float* dx, long long n, wm_stream_t stream);
/* step >= 1 is the 1-based update count; bias corrections are formed in double (torch.optim.Adam semantics) */
int wm_adam_step(float* p, const float* g, float* m, float* v, long long n, double lr, double beta1, double beta2, double eps,
                 int step, wm_stream_t stream);

/* ---- main14b_2 deep-residual variant (py/main14b_2.py:83-224, BASELINE config 5): generic-shape convolutions -------
 * y[nb][co][t'] = act(bias[co] + vec[nb][co] + res[..] + sum_{ci,k} wp[ci*K+k][m] * x[nb][ci][n*S + k - P])
 *   st == 1: m = co, t' = n  (strided Conv1d :87-92, nn.Linear :134, Conv1d k7 :121,:139,:153)
 *   st  > 1: m = co*st + phase, t' = n*st + phase - shp  (ConvTranspose1d(k=2*st, stride st, padding st/2) :147 as a
 *            2-tap convolution + pixel shuffle).  act: 0 none | 1 ELU (:90) | 2 multiply by ELU'(y) with y read from `res` (the
 *            data gradient of the convolution behind an ELU, py/main14b_2.py:96-97, leaves the kernel as dL/dz).  wp is packed by the host mirror. */
/* x2 / Cin1 (optional, NULL / 0): input channels >= Cin1 are the rows of a second tensor x2 [NB][Cin - Cin1][Lin] -- two
 * gradients contracted by one launch (a strided Conv1d and its 1x1 skip conv into the same dL/dx).  nph (0 = st): phases per
 * output channel when st > 1 (m = co*nph + phase, phase < nph <= st): a strided convolution's data gradient only has K phases. */
int wm_gconv(const float* x, const float* wp, const float* bias, const float* vec, const float* res, float* y, int NB,
             int Cin, int Lin, int K, int S, int P, int Mtot, int Nout, int st, int shp, int Cout, int Lout, int act,
             const float* x2, int Cin1, int nph, wm_stream_t stream);
/* wm_gconv on the f16 two-piece split (three f16 piece products per product on v_mfma_f32_32x32x16_f16, fp32 accumulate, fp32-grade):
 * same arguments with wph = wm_gconv_pack_h's image of the SAME wp instead of wp; needs Cin % 16 == 0 (and Cin1 % 16 == 0 with a second
 * source).  gscale = {gs, 1 / gs} (wm_gscale_absmax) -- x is multiplied by gs before the split and clamped to +-6e4 --, NULL: split
 * unscaled. */
int wm_gconv_h(const float* x, const void* wph, const float* bias, const float* vec, const float* res, float* y, int NB,
               int Cin, int Lin, int K, int S, int P, int Mtot, int Nout, int st, int shp, int Cout, int Lout, int act,
               const float* x2, int Cin1, int nph, const float* gscale, float* ymax, int per_clip, wm_stream_t stream);
/* ymax (optional, ONE float zeroed by the caller): receives max |y| over everything the launch stores (atomic max) -- the gradient scale
 * of whatever consumes y next comes from wm_gscale_from_max(ymax, 1, ...) instead of a pass over y.
 * per_clip = 1: gscale holds max |x| per clip ([NB]: a producer's ymax, or wm_absmax_rows) and the kernel splits clip nb times the power
 * of two that puts it into (2^11, 2^12]; ymax receives one maximum per clip ([NB] floats zeroed by the caller) -- activations: an
 * unscaled split loses the lo piece below |x| ~ 2^-3 (f16 subnormals) and saturates above 6e4 */
/* wph: 2 * Cin * K * Mtot f16 ([piece][Cin / 16][K][Mtot][16]: w * ws) followed by {ws, 1 / ws} as two floats.  scratch (>= 1024 floats):
 * ws = the power of two with max |w| ws in (2^9, 2^10] (a pass over wp); scratch NULL: ws = 2^8 fixed, one launch -- what the host mirror
 * uses: the scale only has to keep the two pieces inside the f16 range, which 2^8 does for max |w| between 4e-6 and 250 */
int wm_gconv_pack_h(const float* wp, void* wph, float* scratch, int Cin, int K, int Mtot, wm_stream_t stream);
/* the same image straight from a Conv1d weight w [Cout][Cin][K], fixed scale 2^8: mode 0 = the forward matrix (wp[ci K + k][co] = w[co][ci][k]),
 * mode 1 = the stride-1 data-gradient matrix (wp[co K + kk][ci] = w[co][ci][K - 1 - kk]); the GEMM channel count (Cin | Cout) % 16 == 0 */
int wm_gconv_pack_h_conv(const float* w, void* wph, int Cout, int Cin, int K, int mode, wm_stream_t stream);
/* generic weight gradient, one stride-1 GEMM with the taps folded into the column index (deterministic: split-K partial
 * tiles in `slab`, then a fixed-order fp64 reduce -- no float atomics):
 *   G[a][b][k] (+)= sum_{nb,t} A[nb][a][t] * Bx[nb][b][t + k - P],  dbias[a] (+)= sum A   (Conv1d stride 1: A = dL/dy,
 *   Bx = input; Linear / LSTM: K = 1).  Strided Conv1d / ConvTranspose1d: re-lay the strided operand with wm_gather_taps
 *   first (K = 1 / K = 2 problems) and let `remap` restore the weight's own order: 0 identity | 1 columns k*r1 + b ->
 *   b*r2 + k (r1 = Cin, r2 = taps) | 2 columns (co*r1 + ph)*2 + q -> co*2*r1 + q*r1 + ph (r1 = stride).
 *   b_clip_stride: floats between clips of Bx (0 = dense), so Bx may be a channel slice.  accumulate: 0 overwrite | 1 add.
 * wm_gwgrad_plan reports the workspace (fp32 elements) `slab` must hold for a problem shape.                            */
int wm_gwgrad_plan(int NB, int Ca, int Cb, int La, int K, long long* slab_floats, wm_stream_t stream);   /* host-only query; stream unused */
int wm_gwgrad(const float* A, const float* Bx, float* G, float* dbias, float* slab, int NB, int Ca, int Cb, int La, int Lb,
              int K, int P, long long b_clip_stride, int remap, int r1, int r2, int accumulate, wm_stream_t stream);
/* y[nb][row][t] = x[nb][c][t*S + k - P] (0 outside the clip), t < Lout, c < C, k < K; order 0: row = k*C + c (tap planes of
 * a strided Conv1d, py/main14b_2.py:87-92) | 1: row = c*K + k (stride phases of a ConvTranspose1d, :147)                */
int wm_gather_taps(const float* x, float* y, int NB, int C, int Lin, int K, int S, int P, int Lout, int order, wm_stream_t stream);
/* dz = g * ELU'(z) from y = ELU(z) (py/main14b_2.py:90,:96,:101) */
int wm_elu_bwd(const float* g, const float* y, float* dz, long long n, wm_stream_t stream);
/* out[c] (+)= sum_{nb,t} x[nb][c][t] in a fixed order (partial: >= 64*C floats of scratch; accumulate 0 | 1);
 * out[row] = sum_t x[row][t] for any row length */
int wm_channel_sum(const float* x, float* out, float* partial, int NB, int C, int L, int accumulate, wm_stream_t stream);
int wm_rowsum_any(const float* x, float* out, int rows, int L, wm_stream_t stream);
/* dense embedding gradient for any width: dtable[idx[b]][:] += dvec[b][:], duplicate ids added in batch order */
int wm_rows_scatter_add(float* dtable, const long long* idx, const float* dvec, int Bn, int dim, int nrows, wm_stream_t stream);
/* [A][C][L] -> [L][C][A]: batch-major <-> time-major sequence layout around nn.LSTM (:137) */
int wm_permute_acl(const float* x, float* y, int A, int C, int L, wm_stream_t stream);
/* one layer of nn.LSTM(hd, hd, num_layers=2) (py/main14b_2.py:137, :165) over all T steps as a chain of per-step launches
 * issued by the launcher (the kernel boundary is the step barrier): gate GEMM on the fp32 matrix cores + cell update.
 * Time-major, batch contiguous.  xp [T][4H][B] = W_ih x_t + b (activations overwrite it when save != 0); whh [4H][H];
 * hs, cs [T+1][H][B], row 0 = zero initial state (caller), h_t = hs[t+1].  H % 32 == 0, H <= 256.                   */
int wm_lstm_seq_fwd(float* xp, const float* whh, float* hs, float* cs, int T, int H, int B, int save, wm_stream_t stream);
/* BPTT of that layer: gates [T][4H][B] activations in -> pre-activation gradients out (in place); dout [T][H][B];
 * whhT = weight_hh^T [H][4H]; dc [H][B] scratch.                                                                     */
int wm_lstm_seq_bwd(float* gates, const float* cs, const float* dout, const float* whhT, float* dc, int T, int H, int B,
                    wm_stream_t stream);

/* ---- file ingest: mono mixdown + sample-rate conversion + 1-s segment padding in one launch ----------------------
 * replaces, for a recording that is not at 16 kHz, `waveform.mean(dim=0, keepdim=True)`, torchaudio.transforms.Resample(sr, 16000)
 * and the zero-padded tail segment of the reference's file-level entry points (py/main16.py:714-760).
 *   x (C, N) channel-major, any C >= 1;  P = orig / gcd, Q = new / gcd;  y[m*Q + i] = sum_{k<W} taps[i][k] * xmono[m*P + first[i] + k - width]
 *   with xmono the channel mean (channels added in float64, rounded once to fp32; 0 outside [0, N)), for the L = ceil(Q*N/P) samples of the result; y[L .. total) = 0, so that with
 *   total = ceil(L / seg_len) * seg_len the output is the [S,1,seg_len] model batch (total = L: no padding).
 *   taps [Q][W] fp32 / first [Q] int32: the compact table of torchaudio's default design (sinc_interp_hann, lowpass_filter_width 6,
 *   rolloff 0.99; width = ceil(6 P / (0.99 min(P, Q)))), each phase's run of non-zero taps, W <= 2*width + P, first[i] + W <= 2*width + P.
 * The additions of one sample run k = 0..W-1 whatever kernel or tile computes it.  Rate pairs whose table does not fit LDS run from a
 * one-thread-per-sample kernel that reads it through the cache.  wm_resample_plan (host-only, tile_periods is a HOST pointer, stream
 * unused) reports the output periods of one LDS tile, 0 when that kernel runs. */
int wm_resample_plan(int P, int Q, int width, int W, long long* tile_periods, wm_stream_t stream);
int wm_resample(const float* x, const float* taps, const int* first, float* y, int C, long long N, int P, int Q, int width, int W,
                long long L, long long total, wm_stream_t stream);

/* The way back of the embed path: delta at the model rate -> the recording's own rate, added to every channel of the untouched recording,
 * one launch (the reference has no counterpart: it returns and saves the watermarked signal at 16 kHz mono).
 *   P = delta rate / gcd, Q = recording rate / gcd; taps [Q][W] / first [Q]: the compact table of the pair (delta rate, recording rate), as
 *   for wm_resample;
 *     up[o]     = sum_{k<W} taps[i][k] * d[m*P + first[i] + k - width]      o = m*Q + i,  0 <= o < N
 *     out[c][o] = x[c][o] + up[o]                                           0 <= c < C
 *   d: flat fp32 of which the first Nd samples count; everything outside [0, Nd) is zero BY PREDICATE -- the buffer behind Nd is never read
 *   and may hold anything, NaN included.  N need not be ceil(Q*Nd/P): samples whose window lies past Nd get up = 0.
 *   x, out (C, N) channel-major, C <= 65536.  ALIASING: out may be x itself (in place); no other overlap between d, x, out and up is allowed.
 *   up (N,) may be NULL: not wanted, not written.
 * up[o] is the single chain fmaf(taps[i][k], d, acc), k = 0..W-1, that wm_resample runs -- it equals wm_resample of d[0 .. Nd) with C = 1 bit
 * for bit, whatever tile, workgroup or kernel computed it -- followed by one fp32 add per channel.  Tiles and the choice between the LDS
 * kernel and the one-thread-per-sample kernel are those of wm_resample_plan(P, Q, width, W).  Rows leave as 16-byte accesses when
 * N % 4 == 0 and x, out and up are 16-byte aligned, as 4-byte accesses otherwise (coalesced either way).  N == 0 returns 0 without a launch. */
int wm_resample_add(const float* d, const float* taps, const int* first, const float* x, float* out, float* up, int C, long long N,
                    long long Nd, int P, int Q, int width, int W, wm_stream_t stream);

/* The filter alone on a batch, every row by itself: the resampling attack of the training graph and its backward, no mixdown, no padding.
 *     y[r][m*Q + i] = sum_{k<W} taps[i][k] * x[r][m*P + first[i] + k - width]      0 <= r < rows,  0 <= m*Q + i < L
 *   x (rows, N), y (rows, L), both contiguous; rows * N and rows * L are 64-bit counts.  Outside [0, N) of ITS OWN row a window reads zero BY
 *   PREDICATE: a neighbouring row's samples are never read.  L is any number of outputs per row, not tied to ceil(Q*N/P): fewer cuts the
 *   row short, samples whose window lies past N are sums of zeros.  taps [Q][W] / first [Q]: a compact table as for wm_resample.
 * Row r is the single chain fmaf(taps[i][k], x, acc), k = 0..W-1, of wm_resample: it equals wm_resample of that row alone with C = 1 bit for bit,
 * whatever tile, workgroup or kernel computed it (tiles are numbered per row from period 0 of that row; LDS kernel or one-thread-per-sample
 * kernel as wm_resample_plan(P, Q, width, W) says).  16-byte accesses where every row start is on the 16-byte grid (base aligned and
 * N % 4 == 0 for x, L % 4 == 0 for y, or rows == 1), 4-byte accesses otherwise.  No atomics: bit-reproducible.
 * THE ADJOINT is the same launch: with the table of the pair transposed (ops.resample_adjoint_table: P' = Q, Q' = P, the same float32 values
 * rearranged) on (dy, rows, L -> N) it computes dx[r][n] = sum_o A[o][n] * dy[r][o], A the (L, N) matrix of one row above.
 * rows == 0 or L == 0 returns 0 without a launch. */
int wm_resample_rows(const float* x, const float* taps, const int* first, float* y, long long rows, long long N, long long L, int P, int Q,
                     int width, int W, wm_stream_t stream);

/* ---- 16-bit save path and main15c codec: biquad section + clamp + 16-bit quantiser in one launch -----------------------
 * replaces the host-only `lowpass_biquad(waveform, sample_rate, cutoff_freq=7000)` -> clamp(-1, 1) -> * 32767 -> .to(torch.int16) of the
 * reference's save_audio (py/main15.py:850-867), and `perceptual_postprocess(x) = round(lowpass_biquad(x, 16000, 7000) * 32767) / 32767`
 * that main15c.ipynb applies to s_w = s + delta in train_one_epoch / validate_one_epoch (its cell "perceptual_postprocess").
 *   x (rows, n) fp32, rows >= 1, n >= 1 (any values), every row filtered on its own from a zero state:
 *     y[u] = b0 x[u] + b1 x[u-1] + b2 x[u-2] - a1 y[u-1] - a2 y[u-2]     as one product and four fmaf in this order of terms, -a1 y[u-1] last;
 *     u = t, or with reverse != 0 u = n-1-t: flip(filter(flip(x))) by index mirroring, the adjoint of the forward filter.
 *   warm >= 0 (<= 1024): rows are cut into chunks of 32 samples (in u); each chunk's recursion starts `warm` samples early from a zero state
 *     (before the row: zeros, so chunks within `warm` of the row start are exact) and the warm-up results are dropped.  The host passes
 *     the smallest warm with (pole radius)^warm <= 2^-40.  warm = -1: exact zero-state recursion, one lane per row.  A sample's bits depend
 *     on x, the coefficients, warm and reverse only -- never on the grid; two launches give identical bits.  No atomics.
 *   clamp != 0: c = clamp(y, -1, 1) (torchaudio's lfilter(clamp=True)), else c = y.
 *   mode 0: out fp32 = c | 1: out fp32 = rintf(c * 32767.0f) / 32767.0f (half to even, IEEE division) | 2: out int16 = (int16)(c * 32767.0f),
 *     truncated toward zero, 2 bytes per sample (needs clamp != 0).
 *   mask_out (optional, not with reverse): bit t % 32 of word t / 32, ceil(n / 32) words per row (the layout of wm_bn_add_relu_mask), set
 *     where |y| <= 1 before the clamp.  mask_in (optional, same layout): x is multiplied by its bit on load -- with reverse this is the
 *     backward of "filter, then clamp" in one launch.
 *   b0 = 1, b1 = b2 = a1 = a2 = 0: the quantiser alone (x is passed on as it is).
 * x, the masks and an fp32 out may start at any multiple of 4 bytes (int16 out: of 2); rows leave as 16-byte (int16: 8-byte) accesses
 * wherever a whole aligned group lies inside the row.  hipErrorInvalidValue before any launch: rows or n < 1, a null x or out, out (or a
 * mask) overlapping x -- a chunk reads x behind itself, so in place is not supported --, warm outside -1..1024, mode 2 without clamp,
 * mask_out with reverse.  wm_biquad_plan (host-only, chunk_len is a HOST pointer, stream unused): the chunk length for this warm, 0 when
 * the one-lane-per-row kernel runs. */
int wm_biquad_plan(int warm, int* chunk_len, wm_stream_t stream);
int wm_biquad(const float* x, void* out, void* mask_out, const void* mask_in, float b0, float b1, float b2, float a1, float a2,
              long long rows, long long n, int warm, int mode, int clamp, int reverse, wm_stream_t stream);

/* ---- channel distortions: per-row gain and white Gaussian noise at a per-row SNR, forward and backward ------------------
 * the "volume changes" and "additive noise" of the reference README's "Robustness Testing" section as a step of the graph (the reference
 * ships no code for them).  x (rows, n) fp32, rows >= 1, 1 <= n <= 2^34, every row on its own:
 *     ms_r = (1/n) sum_t x[r][t]^2      g_r = 10^(gain_db_r / 20)      s_r = |g_r| sqrt(ms_r) 10^(-snr_db_r / 20)   (0: the row gets no noise)
 *     y[r][t] = g_r x[r][t] + s_r z(seed, draw, row0 + r, t)            as fmaf(s_r, z, g_r * x); g_r * x alone where s_r == 0
 *   so the SNR of a noisy row is snr_db_r.  0 dB is exactly 1: gain_lo = gain_hi = 0 with p_noise = 0 hands x on bit for bit.
 *   z: Philox4x32-10, key (seed low word, seed high word), counter (q low, q high, row0 + r, draw), q = t >> 2; its words o0..o3 give
 *     u = ((o >> 9) + 0.5) * 2^-23 and samples 4q, 4q+1 = sqrt(-2 ln u(o0)) * (cos, sin)(2 pi u(o1)), 4q+2, 4q+3 the same from (o2, o3), with
 *     the accurate logf / sincospif; |z| <= 5.77.  Nothing of it is stored: the backward call regenerates it.
 *   The row's parameters are drawn in the kernel from the counter (0xFFFFFFFF, 0xFFFFFFFF, row0 + r, draw), which no sample has:
 *     gain_db_r = fmaf(gain_hi - gain_lo, u(o0), gain_lo), snr_db_r = fmaf(snr_hi - snr_lo, u(o1), snr_lo), noise iff u(o2) < p_noise
 *     (lo == hi: a fixed value; p_noise = 0: gain only).  0 <= row0, row0 + rows <= 2^32, 0 <= draw < 2^32; seed: any 64 bits.
 *   stat (rows, 4) fp32 out: {g_r, s_r, ms_r, snr_db_r or +inf where the row got no noise}.
 *   scratch: wm_distort_plan(rows, n) fp32 elements (host-only query, scratch_floats is a HOST pointer, stream unused), caller-allocated.
 * A sample's bits depend on x, the scalars, seed, draw, row0 + r and t only -- never on the grid or on the rows of the launch: rows [0, R) in
 * one call equal R one-row calls with row0 = r.  No atomics.  ms_r is added in one order, a function of n: segments of 16384 samples, in
 * each 256 lanes over the row's quads i, i + 256, ... with one fmaf chain per position in the quad, (c0 + c1) + (c2 + c3), the xor butterfly
 * 32..1 over a wave, waves 0 + 1 + 2 + 3; the segment totals of a longer row (one workgroup each) by one wave, lane j over segments j, j + 64, ...
 * and the same butterfly.  One call enqueues the sum kernel, for n > 16384 the kernel that adds segment totals, and the apply kernel.
 * x, y, stat and scratch may start at any multiple of 4 bytes; y leaves as 16-byte accesses wherever a whole aligned group lies inside the
 * row, and x is read so when it shares y's alignment (the sums read a row that does not start on a 16-byte boundary by 4-byte loads: their
 * order counts quads from the row start).  IN PLACE IS REFUSED: y (dx) may not overlap x (dy, x).
 * wm_distort_bwd, for the same (rows, n, row0, seed, draw) and the stat of the forward call:
 *     dx[r][t] = g_r dy[r][t] + through * (s_r x[r][t] / (n ms_r)) * sum_u dy[r][u] z(.., u)
 *   the second term 0 where ms_r == 0 or the row had no noise; the row sum in the order above (fmaf(dy, z, chain)).  through = 0: the noise level
 *   is a constant, dx = g_r * dy bit for bit, and z is not generated.
 * hipErrorInvalidValue before any launch: rows or n < 1, n > 2^34, row0 or draw out of range, a null or misaligned pointer, p_noise outside
 * [0, 1], a non-finite bound, lo > hi, overlapping input and output. */
int wm_distort_plan(long long rows, long long n, long long* scratch_floats, wm_stream_t stream);
int wm_distort(const float* x, float* y, float* stat, float* scratch, long long rows, long long n, long long row0, long long seed,
               long long draw, float gain_lo, float gain_hi, float snr_lo, float snr_hi, float p_noise, wm_stream_t stream);
int wm_distort_bwd(const float* dy, const float* x, const float* stat, float* dx, float* scratch, long long rows, long long n,
                   long long row0, long long seed, long long draw, int through, wm_stream_t stream);

/* ---- transform-codec stand-in: lapped MDCT, per-band quantiser, bandwidth cut, synthesis -- forward and adjoint in one entry point ----
 * the "compression" of the reference README's "Robustness Testing" section as a step of the graph (the reference ships no code for it).
 * It is the signal path lossy codecs share, NOT an MP3 or AAC encoder: parity with a real encoder is unmeasured.
 * x (rows, n) fp32, rows >= 1, 1 <= n <= 2^34, every row on its own:
 *   Frames.    hop M in {128, 256, 512}; window w[j] = sin(pi (j + 1/2) / (2M)), j < 2M; the row is extended by zeros; F = ceil(n / M) + 1 frames,
 *              frame f holds samples (f-1)M .. (f+1)M - 1, zero outside [0, n).
 *   Analysis.  X_f[k] = sum_j w[j] x_f[j] cos(pi/M (j + 1/2 + M/2)(k + 1/2)), k < M; coefficients k >= kcut are set to 0 (kcut a multiple of band,
 *              band <= kcut <= M); where mask_in (optional, (rows, F, M) int16) holds 0 the coefficient is set to 0 as well.
 *   Quantiser  (quantise != 0).  Bands are `band` consecutive coefficients, band in {4, 8, 16, 32}; in frame f, band b:
 *              P = mean of X^2 over the band (one fmaf chain in rising k, divided by band)
 *              step = max(sqrt(12 P) * 10^(-snr_db_r / 20), floor_step)        q = rint(X / step), ties to even        Xq = q * step
 *              snr_db (rows,) fp32 on the device, 0 <= snr_db_r <= 60 (values outside are clamped to that range, NaN to 0); floor_step > 0.
 *              |q| <= sqrt(band / 12) * 10^3 < 32767: codes_out (optional, (rows, F, M) int16) receives q (0 for k >= kcut).
 *              quantise == 0: Xq = X, the linear map A = synthesis . cut/mask . analysis alone (snr_db is not read; codes_out must be null).
 *   Synthesis. y_f[j] = (2/M) w[j] sum_k Xq_f[k] cos(same argument), overlap-added; y[t] is returned for t < n.
 * With the quantiser off and kcut = M this is the identity (Princen-Bradley), and A is symmetric with or without cut and mask: the backward
 * pass of y = A x is the same launch on dy.  "straight-through" gradient: dx = A dy; "dead zone": dx = A_mask dy with the forward's codes as
 * mask_in (coefficients coded 0 pass nothing).  The step's own dependence on x is not differentiated.
 * One launch; the spectrum stays in LDS (csrc/mdct_codec.hip: fold to DCT-IV, fp32 MFMA).  A workgroup transforms W = 32 or 64 consecutive
 * frames of one row and owns the W - 1 hops between them; the frame two workgroups share is computed by both, each coefficient in one fixed
 * order that knows neither the frame's column nor W.  wm_mdct_codec_plan (host-only, both outputs are HOST pointers, stream unused): W and
 * the workgroups per row for (n, M) -- the W with the fewest padded frames, 32 at M = 512.
 * No atomics, no scratch: a sample's bits depend on its row's data and the scalars only -- never on the grid or on the other rows of the launch.
 * x, y, snr_db may start at any multiple of 4 bytes, the int16 arrays of 2.  IN PLACE IS REFUSED.
 * hipErrorInvalidValue before any launch: rows or n < 1, n > 2^34, M / band / kcut outside the sets above, a non-finite or non-positive
 * floor_step, a null x, y or snr_db, a misaligned pointer, codes_out without quantise, overlapping input and output. */
int wm_mdct_codec_plan(long long n, int M, int* frames_per_workgroup, long long* workgroups_per_row, wm_stream_t stream);
int wm_mdct_codec(const float* x, float* y, void* codes_out, const void* mask_in, const float* snr_db, long long rows, long long n, int M,
                  int band, int kcut, float floor_step, int quantise, wm_stream_t stream);

/* ---- reverb / echo: per-row causal FIR convolution and its adjoint in one entry point; synthetic room responses ---------------------
 * the long convolutive channel (a room, a loudspeaker-microphone path, an echo) as a step of the graph (the reference ships no code for it).
 * x, y (rows, n) fp32, rows >= 1, 1 <= n <= 2^34, every row on its own.  h: K taps per row, 1 <= K <= 16384; row r uses h + r * h_stride,
 * h_stride >= K for per-row responses or 0 for one response shared by all rows.
 *   reverse == 0:  y[r][t] = sum_{k < K, k <= t} h_r[k] x[r][t - k]     the first n samples of the full convolution; lag 0 stays at lag 0
 *   reverse != 0:  y[r][t] = sum_{k < K, t + k < n} h_r[k] x[r][t + k]  = flip(H flip(x)) by index mirroring; H is lower-triangular Toeplitz,
 *                  so this is exactly H^T, the backward pass of the forward map.  h is a constant of both.
 *   Samples outside [0, n) of a row's own data are zero by predicate (a neighbouring row is never read); K may exceed n.
 *   Order.  With t = 32 T + j (mirrored t for reverse) a sample is ONE fp32 fmaf chain from +0 over d = 0, 1, .. and inside d over m = 0 .. 31 of
 *     h[32 d + j - m] * x[32 (T - d) + m], where a tap index outside [0, K) or a sample outside the row contributes an exact zero and lag blocks
 *     d > T (wholly before the row start) may be left out.  With finite data these zeros change nothing, so the chain is the K products
 *     in rising d, rising m.  h = {1} hands x on bit for bit (a -0 leaves as +0).  With finite taps a sample's bits depend on its row's x, its
 *     taps, K, n, reverse and t only -- never on the grid, the other rows of the launch, or whether h is shared: rows [0, R) in one call equal R
 *     one-row calls, and a shared h equals the same h copied per row.
 * One launch (csrc/fir_rows.hip: 32 x 32 Toeplitz blocks on the fp32 MFMA, x and taps in LDS).  No atomics, no scratch.  x, h, y may start at
 * any multiple of 4 bytes.  IN PLACE IS REFUSED.
 * hipErrorInvalidValue before any launch: rows, n or K out of range, h_stride neither 0 nor >= K, a null or misaligned pointer, y overlapping
 * x or h. */
int wm_fir_rows(const float* x, const float* h, float* y, long long rows, long long n, int K, long long h_stride, int reverse,
                wm_stream_t stream);

/* wm_rir_synth: h (rows, K) fp32 out, one synthetic room response per row from params (rows, 2) fp32 on the device, {rt60_s, drr_db} per row.
 * It is exponentially decaying Gaussian noise behind a direct tap -- NOT a room simulation.  1 <= K <= 16384, sample_rate > 0.  For row r:
 *     c = 3 ln 10 / (rt60_r * sample_rate)                 e[0] = 0,  e[k] = z_k * exp(-k c), 1 <= k < K      E = sum_k e[k]^2
 *     w = 10^(-drr_r / 10)     a = sqrt(w / E)             h[0] = 1 / sqrt(1 + w),  h[k] = (a / sqrt(1 + w)) e[k]
 *   so the direct-to-reverberant energy ratio is drr_db, the amplitude decays 60 dB in rt60 and the total energy is 1: white input keeps its
 *   power.  K = 1, E = 0, rt60 not > 0 or a non-finite drr_db give h = {1, 0, ...}; drr_db is clamped to [-100, 100].
 *   z_k: the Box-Muller normal of wm_distort for "sample" k of the counter (k >> 2, 0xFFFFFFFE, row0 + r, draw), key (seed low, seed high), the
 *     four words used as for samples.  No other draw has that counter: wm_distort's samples have high word 0, its parameter counter both
 *     words 0xFFFFFFFF.
 *   Arithmetic: c, k c, exp, w, a and 1 / sqrt(1 + w) in fp64 from the fp32 inputs; exp(-k c) is rounded to fp32 and e[k] is one fp32 product; E is
 *     added in fp32 in the order of wm_distort's sums (256 lanes over the quads i, i + 256, ..., one fmaf chain per position in the quad,
 *     (c0 + c1) + (c2 + c3), the xor butterfly 32..1, waves 0 + 1 + 2 + 3); h[k] = (float)(a / sqrt(1 + w)) * e[k], one fp32 product.
 *   A row's taps depend on (seed, draw, row0 + r, params_r, K, sample_rate) only: rows [0, R) in one call equal R calls with row0 = r.
 * hipErrorInvalidValue before any launch: rows or K out of range, row0 or draw out of range (as wm_distort), a non-finite or non-positive
 * sample_rate, a null or misaligned pointer, params overlapping h. */
int wm_rir_synth(const float* params, float* h, long long rows, int K, float sample_rate, long long row0, long long seed, long long draw,
                 wm_stream_t stream);

/* ---- speed change, wow / flutter and a cut at the front: time warp through a windowed-sinc interpolator, and its adjoint ---------------
 * the desynchronising channel (the reference ships no code for it): the output reads the input at a position that advances `a` input
 * samples per output sample, wobbles sinusoidally and starts `off` samples in.  The output keeps the input's length.
 * x, y (rows, n) fp32, rows >= 1, 1 <= n <= 2^34, every row on its own.  params (rows, 6) fp32 on the device, {a, off, d, w, phi, c} per row:
 *   a speed, off start position in samples, d / w / phi flutter depth in samples / rate in cycles per sample / phase in cycles, c the
 *   anti-alias cutoff relative to Nyquist, clamped to [1/4, 1] (NaN: 1); c32 the clamped fp32 value, c the same number in fp64.
 * tab: zeros * res + 2 fp32 values from the caller, the half response at `res` points per zero crossing over `zeros` zero crossings
 *   (Z = zeros in 4..32, R = res a power of two in 64..1024, (Z R + 2) * 4 <= 128 KiB).
 *   p(t) = fma(a, t, off) + d * sinpi(2 * frac(fma(w, t, phi)))      in fp64 from the fp32 parameters and the integer t, frac(v) = v - floor(v);
 *                                                                    d == 0: the first fma alone
 *   W(u):  v = c * |u|,  s = v * R,  i = floor(s)  (all fp64),  f = (float)(s - i);   W = c32 * fmaf(f, tab[i + 1] - tab[i], tab[i])   in fp32
 *   adjoint == 0:  y[r][t] = sum over k in [0, n) with c |p(t) - k| < Z  of  W(p(t) - k) * x[r][k]      u = p(t) - k is one fp64 subtraction,
 *                  ONE fp32 fmaf chain from +0 in rising k
 *   adjoint != 0:  y[r][k] = sum over t in [0, n) with c |p(t) - k| < Z  of  W(p(t) - k) * x[r][t]      the transposed map with the identical
 *                  fp32 weights, ONE fp32 fmaf chain from +0 in rising t: a gather, never a scatter
 *   The predicate is v < Z on the fp64 v of W, so i <= Z R - 1.  Samples outside [0, n) of a row's own data are never read (a neighbouring
 *   row is never touched).
 *   The adjoint is DEFINED FOR p STRICTLY INCREASING with 0 < a and all parameters finite: the terms of one sample are then one interval of
 *   t, found from the bracket (k -+ (Z / c + 1 + |d|) - off) / a by bisection on p and left at the first p(t) - k > Z / c + 1, and at
 *   most 4096 terms are taken (Z / c <= 128: a slope of p of 1 / 15 or more never has as many).  A row with a <= 0 or a non-finite
 *   parameter gets zeros from the adjoint, and for p not increasing terms may be missing.  The forward map follows the formulas for any
 *   parameters.  WHATEVER params HOLDS -- NaN, infinities, a <= 0 -- every access stays inside x, y, params and tab, and a sample costs
 *   a bounded number of steps: only the values of such a row are unspecified.
 *   With a = 1, integer off, d = 0, c = 1 and a table whose entries at multiples of R are exactly {1, 0, 0, ...}, y is x shifted by off bit
 *   for bit (a -0 leaves as +0), zeros where the shift runs out of the row.
 *   A sample's bits depend on its row's data, its row's parameters, tab, n and its index only -- never on the grid or on the other rows
 *   of the launch; two launches give identical bits.
 * One launch (csrc/time_warp.hip: the table in LDS, one lane per output sample), stateless, enqueue-only.  No atomics, no scratch.  x, params,
 * tab, y may start at any multiple of 4 bytes.  IN PLACE IS REFUSED.
 * hipErrorInvalidValue before any launch: rows, n, zeros or res out of range, a table above 128 KiB, a null or misaligned pointer, y
 * overlapping x, params or tab. */
int wm_time_warp(const float* x, const float* params, const float* tab, float* y, long long rows, long long n, int zeros, int res,
                 int adjoint, wm_stream_t stream);

/* ---- pitch-preserving time stretch: waveform-similarity overlap-add (WSOLA), and its adjoint at constant positions -------------------
 * the other desynchronising channel (the reference ships no code for it): the time axis is stretched by `rate` while the spectrum stays,
 * by copying frames of the input to evenly spaced places of the output, each frame taken near its nominal place where it continues the
 * one before best, cross-faded over half a frame.  Verhelst and Roelands, "An overlap-add technique based on waveform similarity (WSOLA)
 * for high quality time-scale modification of speech", ICASSP 1993.  A pitch shift at constant tempo is this followed by wm_time_warp.
 * x (rows, n_in) fp32, y (rows, n_out) fp32, rows >= 1, 1 <= n_in, n_out <= 2^30, rows * max(n_in, n_out) <= 2^46, every row on its own;
 * xe is x extended by zeros outside [0, n_in).  L (the frame) a power of two in 64..1024, Hs = L / 2 (the hop), 1 <= S <= Hs (the search
 * range).  win: Hs fp32 values from the caller, the rising half window (the package's: float32(0.5 - 0.5 cos(pi j / Hs)) formed in fp64,
 * entry 0 exactly 0).  rate (rows,) fp32 on the device: input samples consumed per output sample, above 1 plays faster.
 * A ROW WHOSE RATE IS NOT FINITE OR LIES OUTSIDE [1/4, 4] GETS ALL ZEROS in y and (mode 0) in delta.  Whatever rate or delta hold, every
 * access stays inside the buffers and a row costs a bounded number of steps.
 *   Frames k = 0 .. K - 1, K = ceil(n_out / Hs) + 1; frame k covers the outputs [o_k, o_k + L), o_k = (k - 1) Hs.
 *   a_k = floor(r o_k + 0.5)   the nominal position: r the fp32 rate as fp64, one fp64 product, one fp64 sum
 *   p_k = a_k + D_k            the chosen position; delta (rows, K) int32 holds D_k; D_0 = 0 (entry 0 is written as 0 and never read)
 *   Search (mode 0, k >= 1, sequential in k):  q = p_(k-1) + Hs is the natural continuation.  For D in [-S, S]
 *       d(D) = sum_{j < L} (xe[q + j] - xe[a_k + D + j])^2
 *     each term one fp32 subtraction and one fmaf.  The order: with P the largest power of two <= min(4096 / S, L / 8) (integer division),
 *     the terms j in [i L / P, (i + 1) L / P) form one fmaf chain from +0 in rising j, and the P chains are added in fp32 in rising i.  It
 *     depends on (L, S) and j alone -- never on the grid, the row count or the other rows.  D_k is the candidate with the smallest fp32
 *     score; ties go to the first candidate in the order 0, -1, +1, -2, +2, ...; a NaN score never wins, and if every score is NaN D_k = 0.
 *     A squared difference and not a cross-correlation: at rate 1 the continuation scores exactly 0, so the map is the identity without a
 *     normalisation, and a sum without cancellation has a purely relative fp32 error.
 *   Synthesis: output t = m Hs + j, 0 <= j < Hs:   u = xe[p_(m+1) + j],  v = xe[p_m + Hs + j],  y[t] = fmaf(win[j], u - v, v)
 *     (u - v one fp32 subtraction).  Linear in x; where p_(m+1) = p_m + Hs it equals x bit for bit.
 *   mode 0: search, write delta, synthesise.
 *   mode 1: synthesise from the caller's delta, every entry clamped to [-S, S] on load.
 *   mode 2: the adjoint of mode 1.  x is the gradient g (rows, n_out), y is dx (rows, n_in); ge is g extended by zeros;
 *       dx[s] = sum over the frames k with 0 <= s - p_k < L  of  W[s - p_k] ge[o_k + s - p_k]
 *       W[i] = win[i] for i < Hs and 1 - win[i - Hs] (one fp32 subtraction) for i >= Hs
 *     ONE fp32 fmaf chain from +0 in rising k, a gather: a_k is monotone and |D| <= S, so the frames of a sample are one bracket of k found
 *     by arithmetic, of at most (L + 2 S) / (Hs / 4) + 3 members.  A term whose output index lies outside [0, n_out) is left out.
 *   A sample's bits depend on its row's data, its row's rate (and delta), win, the dimensions and its index only; two launches give
 *   identical bits.
 * One launch (csrc/wsola.hip: mode 0 one workgroup per row with the frame's template and candidates in LDS, modes 1 and 2 one lane per
 * sample), stateless, enqueue-only.  No atomics, no scratch.  Every pointer may start at any multiple of 4 bytes.  IN PLACE IS REFUSED.
 * hipErrorInvalidValue before any launch: rows, n_in, n_out, L or S out of range, mode outside 0..2, a null or misaligned pointer, y
 * overlapping x, rate, win or delta, and in mode 0 delta overlapping x, rate or win. */
int wm_wsola(const float* x, const float* rate, const float* win, float* y, int* delta, long long rows, long long n_in, long long n_out,
             int L, int S, int mode, wm_stream_t stream);

/* ---- predictive speech-codec stand-in: per-frame LPC, open-loop residual quantiser, all-pole synthesis -- and the adjoint -------------
 * the channel a speech recording most likely crosses (ADPCM, CELP, AMR-WB, SILK are all linear-predictive) as a step of the graph; the
 * reference ships no code for it.  White quantisation noise goes on the prediction residual and the synthesis filter shapes it like the
 * frame's spectral envelope.  It is a STAND-IN, not a speech codec: open-loop quantisation, no LSP interpolation, no pitch predictor, no
 * noise feedback, no entropy coder; parity with any real codec is unmeasured.
 * x, y (rows, n) fp32, rows >= 1, 1 <= n <= 2^34, rows * n <= 2^46, every row on its own; xe is the row extended by zeros.  Frame length
 * L in {160, 320, 640}, order p in 2..16, F = ceil(n / L) frames, frame f owns the samples fL .. (f+1)L - 1, f(t) = floor(t / L).
 *   Analysis (coeffs_in null).  w[j] = 0.5 - 0.5 cos(2 pi (j + 1/2) / (2L)), j < 2L, evaluated in fp64 and rounded once to fp32.
 *       s[j]  = w[j] * xe[fL - L/2 + j]                      one fp32 product
 *       R[k]  = sum_{j < 2L - k} s[j] s[j + k], k <= p        64 fmaf chains from +0, chain l over j = l, l + 64, ... rising; the chains are
 *                                                            added by the xor butterfly 32, 16, .. 1 (v += partner: the same bits in every lane)
 *       Rc[k] = R[k] * lag[k]                                lag (p + 1,) fp32 on the device, from the caller (the package's: lag[0] = 1 + 1e-4,
 *                                                            the white-noise correction, lag[k] = exp(-0.5 (2 pi 60 k / sample_rate)^2), in fp64,
 *                                                            rounded once)
 *     Levinson-Durbin in fp32 on Rc, a all 0 at the start.  !(Rc[0] > 0): the frame's coefficients stay 0.  E = Rc[0]; at step i = 1 .. p:
 *       acc = Rc[i], then acc = fmaf(a_j, Rc[i - j], acc) for j = 1 .. i - 1 rising;  k_i = -acc / E (one IEEE division).
 *       !(|k_i| < 1): the recursion stops, a_j = 0 for j >= i.  Otherwise a_j <- fmaf(k_i, a_(i-j), a_j) for j < i (from the old values),
 *       a_i = k_i,  E <- E * fmaf(-k_i, k_i, 1).
 *     Then a[k] <- a[k] * expand[k - 1], expand (p,) fp32 on the device from the caller (the package's: 0.994^k, k = 1 .. p, in fp64).
 *     coeffs_in ((rows, F, p) fp32, optional) replaces all of this; coeffs_out (optional, same shape) receives exactly the fp32
 *     coefficients the launch used.  lag and expand are read only without coeffs_in.
 *   Residual.   e[t] = x[t] + sum_{k = 1..p} a_f(t)[k] xe[t - k]     one fmaf chain from x[t] in rising k; the predictor runs on the INPUT
 *   Quantiser (quantise != 0), per frame:
 *       P = (sum of e^2 over the frame's samples inside the row) / their number; the sum: 64 fmaf chains from +0, chain l over the frame's
 *           samples l, l + 64, ... rising, the same butterfly
 *       step = max(sqrt(12 P) * g, floor_step),  g = 10^(-snr_db_r / 20) in fp64 rounded once;  snr_db (rows,) fp32 on the device, clamped to
 *           0..60, NaN to 0;  floor_step > 0 (the package's: 2^-15)
 *       q = rint(e / step), ties to even (one IEEE division)        eq = q * step
 *       |q| <= sqrt(L / 12) * 10^3 < 32767: codes_out (optional, (rows, n) int16) receives q.   quantise == 0: eq = e (snr_db is not read).
 *     Where mask_in (optional, (rows, n) int16) holds 0, eq[t] = 0.
 *   Synthesis.  y[t] = eq[t] - sum_{k = 1..16} a_f(t)[k] y[t - k],  y[< 0] = 0, a[k] = 0 for k > p: one fmaf chain from eq[t] in FALLING k,
 *       fmaf(-a[k], y[t - k], acc), so the newest output enters last.  (The zero terms change no bit of a finite result.)
 *     With the quantiser off and no mask y = x up to rounding: synthesis inverts the residual filter.
 *   adjoint != 0 (needs coeffs_in; quantise == 0, no coeffs_out, no codes_out): x is the gradient g, y is dx, the transpose of the linear
 *     map y = S M A x at these coefficients (A the residual filter, M the mask, S synthesis), the coefficient taken at the ROW index of each
 *     matrix -- the frame of the sample the term comes FROM.  For t falling from n - 1:
 *       u[t]  = g[t] - sum_{k = 1..16} a_f(t+k)[k] u[t + k]          one fmaf chain from g[t] in FALLING k, as the synthesis
 *       v[t]  = mask[t] * u[t]                                      (mask 1 or 0; all 1 without mask_in)
 *       dx[t] = v[t] + sum_{k = 1..p} a_f(t+k)[k] v[t + k]           one fmaf chain from v[t] in rising k
 *     terms with t + k >= n are left out (they are exact zeros).
 *   The order of every sum depends on (L, p) and the index alone.  A sample's bits depend on its row's data, the tables and the scalars
 *   only -- never on the grid or on the other rows of the launch; two launches give identical bits.
 * One launch (csrc/lpc_codec.hip: one workgroup per row; producer waves analyse and quantise a chunk of frames ahead into an LDS ring,
 * one wave runs the recursion, the producers write the chunk behind it out), stateless, enqueue-only.  No atomics, no scratch.  The fp32
 * arrays may start at any multiple of 4 bytes, the int16 arrays of 2.  IN PLACE IS REFUSED: no output may overlap an input or another
 * output.
 * hipErrorInvalidValue before any launch: rows or n out of range, L or p outside the sets above, a null x or y, a misaligned pointer, no
 * coeffs_in and a null lag or expand, quantise with a null snr_db or a non-finite or non-positive floor_step, codes_out without
 * quantise, adjoint without coeffs_in or with quantise, coeffs_out or codes_out, overlapping buffers. */
int wm_lpc_codec(const float* x, float* y, const float* coeffs_in, float* coeffs_out, void* codes_out, const void* mask_in,
                 const float* snr_db, const float* lag, const float* expand, long long rows, long long n, int L, int p, float floor_step,
                 int quantise, int adjoint, wm_stream_t stream);

/* ---- STOI: short-time objective intelligibility (Taal, Hendriks, Heusdens, Jensen 2011) of a processed signal against its reference ----
 * replaces the per-segment pystoi.stoi(clean, wm, 16000, extended=False) loop of evaluate_unseen_file (py/main14.py:1099-1203,
 * py/main16.py:2012-2153) at the rate the measure is defined at.  x (the reference) and y (the processed signal) are (rows, n) fp32 AT
 * 10 kHz, rows >= 1, 1 <= n <= 2^34, every row pair scored on its own.  EPS = 2^-52.  Extended STOI is not built.
 *   1 window    w[t] = 0.5 (1 - cos(2 pi (t + 1) / 257)), t = 0..255   (numpy.hanning(258)[1:-1])
 *   2 frames    frame f starts at 128 f for every f with 128 f < n - 256: F = max(0, ceil((n - 256) / 128)) frames (the bound is strict: a
 *               row of exactly 256 samples has none);  xf_f[t] = w[t] x[128 f + t], the same for y
 *   3 silence   decided on x alone: frame f is kept iff ||xf_f|| + EPS > 0.01 (max_g ||xf_g|| + EPS) -- "more than 40 dB below the loudest
 *               frame" without the logarithm; an all-zero row keeps every frame.  K kept frames with start samples s_0 < ... < s_(K-1);
 *               they are overlap-added at hop 128 into xs, ys of length 128 (K - 1) + 256:  xs[128 h + t] += w[t] x[s_h + t], ys with the
 *               same s_h
 *   4 spectra   frames of xs / ys by rule 2 again: S = K - 1 of them (the last hop has none), windowed by w again, zero-padded to 512,
 *               one-sided DFT; bins 7..218 are used
 *   5 bands     J = 15 third-octave bands, band b sums |X[k]|^2 over k in [lo_b, hi_b), the bins nearest to 150 * 2^((2b -+ 1) / 6) Hz on the
 *               grid k * 10000 / 512:  (7,9) (9,11) (11,14) (14,17) (17,22) (22,27) (27,34) (34,43) (43,55) (55,69) (69,87) (87,109)
 *               (109,138) (138,174) (174,219);  X_b[j] = sqrt(sum), the same for Y
 *   6 segments  S < 30: d = 1e-5, the published sentinel.  Else segment m = 30..S is frames m - 30 .. m - 1; per band and segment, with the
 *               30-vectors xi, eta:  alpha = ||xi|| / (||eta|| + EPS);  eta' = min(alpha eta, (1 + 10^(15/20)) xi);  the means of xi and
 *               eta' are removed, each is divided by (its norm + EPS);  rho = <xi, eta'>.  d = the mean of rho over all J (S - 29) pairs
 *   7 output    d[r] fp32 and kept[r] = K as an int.  An all-zero x or an all-zero y gives exactly d = 0.  A row with a non-finite sample
 *               anywhere in x or y (or a frame energy beyond fp32) gives d = NaN and kept = 0, for that row only.
 * Computed in fp32 (csrc/stoi.hip): five launches -- frame norms, the kept-frame list, band magnitudes through one complex 512-point
 * transform per frame pair (x real, y imaginary), segment correlations, the mean -- all sized for F; K never reaches the host.  No atomics:
 * a row's bits depend on its samples and n only, never on rows, its place in the batch or the grid; two launches give identical bits.
 * Whatever the data holds, every index stays inside the row and every loop is capped by F.
 * scratch: wm_stoi_plan(rows, n) BYTES (host-only query, scratch_bytes is a HOST pointer, stream unused), caller-allocated, contents
 * unspecified before and after.  x, y, d, kept, scratch may start at any multiple of 4 bytes; inputs are borrowed.
 * hipErrorInvalidValue before any launch: rows or n out of range, rows * n > 2^46, a null or misaligned pointer, d, kept or scratch
 * overlapping an input or one another. */
int wm_stoi_plan(long long rows, long long n, long long* scratch_bytes, wm_stream_t stream);
int wm_stoi(const float* x, const float* y, float* d, int* kept, void* scratch, long long rows, long long n, wm_stream_t stream);

/* ---- spectral masking: noise-to-mask ratio of a processed signal against its reference, and the masking loss with its gradient -------
 * The reference's README speaks of a watermark "below psychoacoustic thresholds" and computes none (TFLoudnessLoss, py/main16.py:204-217,
 * is a gated squared magnitude difference).  This is ONE simultaneous-masking model of the 1988 kind -- Bark bands, the Schroeder spreading
 * function, Johnston's tonality offset, Terhardt's threshold in quiet -- at an ASSUMED playback level (a full-scale sine = 96 dB SPL).  No
 * temporal masking; the mask is not differentiated; parity with PEAQ, with an MPEG encoder's model and with listeners is unmeasured.
 * x (the reference) and y (the processed signal) are (rows, n) fp32 AT 16 kHz, rows >= 1, 1 <= n <= 2^34, rows * n <= 2^46; every row
 * pair on its own; d = y - x.
 *   1 frames     N = 512, hop 256, periodic Hann w[t] = 0.5 (1 - cos(2 pi t / 512)), no padding: F = 1 + (n - 512) / 256 (integer division)
 *                for n >= 512, else 0.  A tail shorter than a hop is not judged and gets zero gradient.
 *   2 power      k = 0..256:  P_v[f,k] = c_k |sum_t w[t] v[256 f + t] e^(-2 pi i k t / 512)|^2,  c_k = 2 (8/3) / 512^2 for 0 < k < 256 and
 *                (8/3) / 512^2 at k = 0 and 256 (8/3 undoes the window's power loss: a full-scale sine sums to about 0.5)
 *   3 bands      z(f) = 13 atan(0.00076 f) + 3.5 atan((f / 7500)^2),  band(k) = min(floor(z(k 16000 / 512)), Z - 1),  Z = floor(z(8000)) + 1
 *                = 22; bins per band: 4 3 3 4 3 4 4 5 5 6 6 8 8 11 13 16 20 23 28 32 38 13 (257 in all).  E_x[f,b], E_d[f,b]: the band sums
 *                of P_x and P_d
 *   4 spreading  S[b,j] = 10^(SF(b - j) / 10),  SF(D) = 15.81 + 7.5 (D + 0.474) - 17.5 sqrt(1 + (D + 0.474)^2);
 *                C[f,b] = sum_j S[b,j] E_x[f,j],  G[b] = sum_j S[b,j]
 *   5 tonality   over bins 1..255 of P_x:  sfm_dB = 10 log10(exp(mean ln(P + 1e-30)) / (mean P + 1e-30)),  alpha = clip(sfm_dB / -60, 0, 1),
 *                O[f,b] = alpha (14.5 + b) + (1 - alpha) 5.5  dB
 *   6 quiet      ath(f) = 3.64 f^-0.8 - 6.5 e^(-0.6 (f - 3.3)^2) + 1e-3 f^4 dB SPL, f in kHz, at the bin centres (bin 0 at bin 1's
 *                frequency);  A[b] = 0.5 * 10^((min over the band's bins of ath - 96) / 10)
 *   7 mask       T[f,b] = max(C[f,b] 10^(-O[f,b] / 10) / G[b], A[b]),  r[f,b] = E_d[f,b] / T[f,b]
 *   8 outputs    nmr_db = 10 log10(mean over f,b of r);  over_db = mean over f,b of max(0, 10 log10 r);  counts[2 row] = audible = #{r > 1},
 *                counts[2 row + 1] = cells = 22 F.  F = 0: NaN, 0, 0, 0.  d == 0: -inf, 0.  A non-finite sample anywhere in the row of x or
 *                y: both floats NaN, both counts 0, for that row only.
 *   9 gradient   d over_db / d y only; the mask is a function of x alone and a constant of the backward pass, x gets no gradient.  With
 *                g[f,b] = (10 / ln 10) / E_d[f,b] where r > 1, else 0 (this is `coef`; E_d > T >= A[b] > 0 there: no division near zero):
 *                  gy[t] = gout[row] / cells * sum_f w[t - 256 f] Re sum_k 2 g[f,band(k)] c_k D[f,k] e^(+2 pi i k (t - 256 f) / 512),
 *                D the windowed spectrum of d.  Samples no frame covers are written as 0.  A row that scored NaN: gy unspecified.
 * tables: ONE device buffer of 1042 words from the caller, formed in float64 and rounded once (the package's masking_tables()):
 *   c_k[257] | band[257] as int32 | S[22][22] | G[22] | A[22].  The window is not among them: both directions form it themselves, the
 *   forward in fp64 (its fp32 rounding alone would cost 5e-7 dB of over_db on a one-frame row).  wm_masking_bwd takes no tables at all:
 *   c_k and band(k) are closed forms too (the bin counts above).
 * coef (nullable, (rows, F, 22) fp32): written by wm_masking_fwd when given, read by wm_masking_bwd (required there when F > 0).
 * The forward is computed in fp64 from the window on (the tables stay fp32), the backward in fp32 (csrc/masking.hip).  Forward: one launch over (row, chunk of `chunk` frames) -- the frames
 * in pairs, two frames of ONE signal per complex 512-point transform -- and one launch that finishes each row in a fixed order.  Backward:
 * one launch over (row, 256 output samples); each workgroup forms the two frames that cover its samples.  No atomics: a row's bits depend
 * on its samples and n only, never on rows, its place in the batch or the grid; two launches give identical bits.
 * wm_masking_plan: host-only query (the three results are HOST pointers, stream unused): frames = F, chunk = the frames one workgroup of
 * the forward handles, scratch_bytes = what `scratch` must hold (caller-allocated, contents unspecified before and after).
 * Every pointer may start at any multiple of 4 bytes; inputs are borrowed.
 * hipErrorInvalidValue before any launch: rows or n out of range, rows * n > 2^46, a null or misaligned pointer (coef may be null in the
 * forward, and in the backward when F = 0), an output overlapping an input or another output. */
int wm_masking_plan(long long rows, long long n, long long* frames, long long* chunk, long long* scratch_bytes, wm_stream_t stream);
int wm_masking_fwd(const float* x, const float* y, const float* tables, float* nmr_db, float* over_db, int* counts, float* coef,
                   void* scratch, long long rows, long long n, wm_stream_t stream);
int wm_masking_bwd(const float* x, const float* y, const float* coef, const float* gout, float* gy, long long rows, long long n,
                   wm_stream_t stream);

/* ---- splice attack and localisation: per-sample labels, the detection losses against them, confusion counts ------------------------
 * the editing attack: part of a watermarked recording is cut out and replaced by unmarked audio, by silence, or by audio moved from
 * elsewhere in the same recording (the reference ships no code for it; its target is all ones on the watermarked half, py/main16.py:255-258).
 * LABEL MASKS, shared by the five entry points: lab (rows, W) 32-bit words (declared int*, read as uint32), W = ceil(n / 32); bit j of word w of row r is sample 32 w + j of row
 *   r; 1 = "still watermarked"; bits at t >= n are zero.  Every mask is formed by wave ballots, one writer per word.
 * wm_splice: a (the watermarked signal) and b (the clean one) (rows, n) fp32, y (rows, n) fp32 out, lab (rows, W) out; rows >= 1,
 *   1 <= n <= 2^24, 1 <= max_spans <= 8, 1 <= len_lo <= len_hi <= n (samples), p_span, p_original, p_silence in [0, 1] with
 *   p_original + p_silence <= 1 (the rest is the probability of "moved"); 0 <= row0, row0 + rows <= 2^32, 0 <= draw < 2^32; seed: any 64 bits.
 *   Span j < max_spans of row r takes two Philox4x32-10 draws, key (seed low word, seed high word) as wm_distort, counters
 *     (0xFFFFFFFB - 2j, 0xFFFFFFFF, row0 + r, draw) -> o0..o3   and   (0xFFFFFFFA - 2j, 0xFFFFFFFF, row0 + r, draw) -> o0'
 *   which no other draw has.  With u(o) = ((o >> 9) + 0.5) * 2^-23 and v(o) = o >> 9:
 *     active iff u(o0) < p_span                               L     = len_lo + ((v(o1) * (len_hi - len_lo + 1)) >> 23)
 *     start = (v(o2) * (n - L + 1)) >> 23                     kind  = original if u(o3) < p_original, silence if u(o3) < p_original + p_silence, else moved
 *     shift = 1 + ((v(o0') * (n - 1)) >> 23)                  (n = 1: moved acts as original)
 *   the thresholds p_span, p_original and p_original + p_silence in fp64 from the fp32 arguments, the products in 64-bit integers: the
 *   geometry has no float rounding and a host restatement agrees to the bit.
 *   Sample t: let j* be the largest active j with start_j <= t < start_j + L_j.  None: y = a[r][t], label bit 1.  Else label bit 0 and
 *   y = b[r][t] (original) | +0 (silence) | b[r][(t + shift) mod n] (moved).  Values are copied bit for bit; a rectangular cut, no crossfade.
 *   A sample's bits depend on its row's data, (seed, draw, row0 + r), the scalars and t only: rows [0, R) in one call equal R one-row calls
 *   with row0 = r; two launches give identical bits.
 * wm_splice_bwd: da = dy where the label bit is 1, else +0, bit for bit.  b is data: it has no gradient.
 * Both: one launch, stateless, enqueue-only, no scratch.  Pointers may start at any multiple of 4 bytes; y (da) leaves as 16-byte accesses
 * wherever a whole aligned group lies inside the row and a, b (dy) are read so where they share that alignment.  IN PLACE IS REFUSED.
 * hipErrorInvalidValue before any launch: rows, n, row0, draw, max_spans, a length or a probability out of range (NaN included), a null or
 * misaligned pointer, an output overlapping an input or the other output.
 *
 * wm_bce_masked_fwd / _bwd: wm_bce_fwd / wm_bce_bwd against the labels.  logits [R][T][NO], message [B] int64, lab (B, ceil(T / 32)) for rows
 *   < B; rows >= B have target 0 throughout; shapes and limits of wm_bce_fwd (T * NO < 2^23, R <= 65535), 0 <= B <= R, NO <= 64.
 *     loc = (1 / (R T)) sum_{r, t} bce(logits[r][t][0], y_rt)                                  y_rt = the label bit for r < B, else 0
 *     bce = (1 / (N1 (NO - 1))) sum_{r < B, t with label 1, o >= 1} bce(logits[r][t][o], bit_(o-1)(message_r))
 *   N1 = the number of set label bits (at t < T): the message can only be decoded where the watermark still is.  It is an integer
 *   popcount, written to count_out (a DEVICE int64) and read from the device by the finish and by the backward call (count): no host
 *   sync.  N1 = 0: bce = 0 and every bit gradient is +0.  NO = 1 leaves bce_out untouched.
 *   partial: >= 3 * R * ceil(T*NO / 4096) 32-bit words of scratch (wm_bce_fwd's two float slabs and one of integer counts).
 *   The fp32 partials per workgroup and their fp64 finish are wm_bce_fwd's, in its order (bit-reproducible run to run); with every label 1
 *   dlogits equals wm_bce_bwd's bit for bit.  The backward has wm_bce_bwd's expressions with y_rt and the scale 1 / (N1 (NO - 1)).
 *   hipErrorInvalidValue before any launch: a shape out of range, a null pointer, dlogits overlapping logits.
 *
 * wm_loc_score: prediction = logits[r][t][0] > thr_logit (NaN predicts 0) against the label bit of lab (lab_rows, ceil(T / 32)); rows >=
 *   lab_rows have label 0; lab == NULL: every label is 1.  counts (R, 4) int32 out = {tp, fp, fn, tn}, exact; pred (optional, (R,
 *   ceil(T / 32)) out): the prediction in the mask layout, tail bits zero.  One launch, one workgroup per row.
 *   hipErrorInvalidValue before any launch: R, T or NO < 1, lab_rows outside [0, R], a NaN threshold, a null logits or counts. */
int wm_splice(const float* a, const float* b, float* y, int* lab, long long rows, long long n, long long row0, long long seed,
              long long draw, int max_spans, float p_span, long long len_lo, long long len_hi, float p_original, float p_silence,
              wm_stream_t stream);
int wm_splice_bwd(const float* dy, const int* lab, float* da, long long rows, long long n, wm_stream_t stream);
int wm_bce_masked_fwd(const float* logits, const long long* message, const int* lab, float* partial, long long* count_out,
                      float* loc_out, float* bce_out, int B, int R, int T, int NO, wm_stream_t stream);
int wm_bce_masked_bwd(const float* logits, const long long* message, const int* lab, const long long* count, const float* g_loc,
                      const float* g_bce, float* dlogits, int B, int R, int T, int NO, wm_stream_t stream);
int wm_loc_score(const float* logits, const int* lab, float thr_logit, int* counts, int* pred, int R, int T, int NO,
                 int lab_rows, wm_stream_t stream);

/* ---- per-clip detection scores: what an operating-point report (ROC, AUC, TPR at a set FPR, message accuracy) needs of the logits ------
 * replaces the per-clip reductions of evaluate_model (py/main16.py:386-403: sigmoid, mean, compare, mean, compare) and feeds what the
 * reference hands to roc_curve / auc / confusion_matrix (py/main16.py:2372-2386) with one pass over the Detector's output.
 * logits [R][T][NO] fp32 contiguous, channel 0 the detection logit, channels 1 .. NO - 1 the message bits; message [B] int64 (optional),
 * bit o - 1 the target of channel o, for the rows r < B; 1 <= T <= 2^24, 1 <= NO <= 64, 0 <= B <= R, R * T * NO <= 2^46.
 * Per row r, with x[t][o] = logits[r][t][o]:
 *   prob[r]        fp32   (1 / T) sum_t sigmoid(x[t][0])                   the reference's per-clip score              (optional)
 *   llr[r][o]      fp32   (1 / T) sum_t x[t][o], o in [0, NO)              the mean log-likelihood ratio               (optional)
 *   votes[r][o]    int32  o = 0: #{t : x[t][0] > thr_logit};  o >= 1: #{t : x[t][o] > 0}                  exact; a NaN is no vote
 *   words[r][0]    int64  bit o - 1 set iff 2 * votes[r][o] > T            the majority of hard decisions; a tie is 0  (optional)
 *   words[r][1]    int64  bit o - 1 set iff sum_t x[t][o] > 0              the soft decision: the sum of log-likelihood ratios, the
 *                                                                          combination the reference does not have; a NaN sum is 0
 *   biterr[r][k]   int32  r < B: popcount((words[r][k] ^ message[r]) & (2^(NO-1) - 1)), k = 0, 1                       (optional)
 *                         B = 0 or message == NULL leaves biterr untouched; NO = 1 writes zeros to words and biterr.
 * The vote is taken on the LOGIT: x > thr_logit with thr_logit = log(p / (1 - p)) from the caller (+-inf allowed: no vote / every
 * non-NaN sample above -inf votes), x > 0 for the bits -- as wm_loc_score does -- not on sigmoid(x) > p in fp32.  The two differ only
 * for 0 < x <~ 2^-23, where the fp32 sigmoid rounds to 0.5 exactly and the reference's comparison says no.  For logits that are 0 or
 * at least 1e-3 in magnitude the integer rule gives the decoded bits of evaluate_model's (mean_t (sigmoid > 0.5)) > 0.5 exactly.
 * Sums.  A row is cut into chunks of 8192 ELEMENTS (of its T * NO; a constant).  Per chunk and channel one fp32 partial: the elements of
 *   the channel are dealt to floor(256 / NO) threads (thread j takes every floor(256 / NO)-th, in rising t, one fp32 chain from +0), and
 *   the threads' sums are added in four chains (j mod 4) in rising j, ((c0 + c1) + (c2 + c3)).  The sigmoids (1 / (1 + expf(-x)), IEEE
 *   division) of a chunk: 256 chains, the wave butterfly 32 .. 1, the four waves in rising order.  The finish adds a row's partials in
 *   fp64: chunks in four contiguous groups of ceil(chunks / 4), inside a group four chains (position mod 4) in rising order, the groups
 *   in rising order; prob's 256 chains (chunk mod 256) by the same butterfly.  prob = (float)(sum / T), llr likewise; the soft bit
 *   tests the finished fp64 sum.  The order depends on (T, NO) alone: a row's bits depend on its own samples, T, NO, thr_logit and its
 *   message -- never on R, the row's place in the batch, the grid or the pointer's alignment.  Rows [0, R) in one call equal R one-row
 *   calls bit for bit; two launches give identical bits.
 * Non-finite samples: a NaN makes prob[r] (channel 0) or llr[r][o] of ITS row and channel NaN and casts no vote; +-inf vote by the
 *   comparison, give sigmoid 1 / 0 and an infinite (or, with both signs, NaN) llr.  No other row or channel changes a bit.
 * Two launches (csrc/clip_scores.hip: one workgroup per (row, chunk) stages the chunk through LDS with 16-byte loads wherever a whole
 * aligned group lies inside it; then one workgroup per row), stateless, enqueue-only, no atomics.  logits may start at any multiple of
 * 4 bytes; message and words at multiples of 8, the rest of 4.
 * scratch: wm_clip_scores_plan(R, T, NO) BYTES (host-only query, scratch_bytes is a HOST pointer, stream unused) =
 *   R * ceil(T * NO / 8192) * (2 NO + 1) * 4; caller-allocated, contents unspecified before and after.
 * hipErrorInvalidValue before any launch: R or T < 1, NO outside [1, 64], B outside [0, R], R * T * NO > 2^46, T > 2^24 (int32 counts,
 * fp32 partials), a NaN thr_logit, a null logits, votes or scratch, a misaligned pointer, an output (scratch included) overlapping an
 * input or another output. */
int wm_clip_scores_plan(long long R, int T, int NO, long long* scratch_bytes, wm_stream_t stream);
int wm_clip_scores(const float* logits, const long long* message, float thr_logit, float* prob, float* llr, int* votes, long long* words,
                   int* biterr, void* scratch, long long B, long long R, int T, int NO, wm_stream_t stream);

/* ---- clip curation: the speech / noise feature table and the silence measure of the dataset scripts, one launch ----------------------
 * replaces analyze_audio_file + classify_speech_noise of dataset_creation/noise.py (librosa 0.10 defaults, scipy) and the rms of
 * dataset_creation/silent.py, which the reference runs per file in a process pool.  x (rows, n) fp32 at sample_rate sr, every row on its
 * own; 400 <= n <= 32768, 6000 < sr <= 2^20, int(0.025 sr) <= n, rows >= 1.  With y = the row and F = 1 + n / 512 (integer division):
 *   feat (rows, 16) fp32, the columns in this order (0..11 are the reference's CSV columns):
 *    0 duration               n / sr
 *    1 energy                 mean(y^2)
 *    2 speech_band_energy     mean(z^2), z = y through the order-5 Butterworth band-pass 300..3000 Hz from zero initial state
 *                             (scipy.signal.butter(5, [300, 3000] / (sr / 2), 'band') + lfilter), run as the five second-order sections
 *                             sos (5, 6) = rows of b0 b1 b2 1 a1 a2, cascaded in the order given, transposed direct form II
 *    3 zero_crossing_rate     y padded by 1024 samples at each end with the EDGE value, F frames of 2048 at hop 512, samples with
 *                             |v| <= 1e-10 set to 0; a position i >= 1 of a frame counts iff signbit differs from position i - 1 (the
 *                             first sample of a frame never counts); rate = total count / (2048 F)
 *    4 spectral_centroid      S = |rfft(frame * periodic Hann 2048)| on y padded by 1024 ZEROS at each end, hop 512, f_k = k sr / 2048;
 *    5 spectral_bandwidth     per frame c = sum f_k S_k / sum S_k, bandwidth = sqrt(sum (S_k / sum S)(f_k - c)^2), roll-off bin = the
 *    6 rolloff                smallest k with cumsum(S)_k >= 0.85 sum S (the feature is its frequency k sr / 2048); a frame whose sum S
 *                             is below fp32 tiny (1.17549435e-38) gives 0 for all three; each feature is the mean over the F frames
 *    7 mfcc_mean              M = S^2 mel^T with fb (1025, 128) fp32 (fb[k][m], 128 Slaney-scale, Slaney-normalised triangles from 0 to
 *    8 mfcc_var               sr / 2, built in fp64 and rounded) of which mel m uses the bins klo[m] .. khi[m] (inclusive; the banded form
 *                             of wm_mel_loss); dB = 10 log10(max(1e-10, M)), clamped from below at (maximum dB of the clip) - 80; the
 *                             first 13 coefficients of the orthonormal DCT-II along the mel axis, dct (13, 128) fp32; mfcc_mean = the
 *                             mean over coefficients of the mean over frames, mfcc_var = the mean over coefficients of the variance
 *                             over frames (ddof 0)
 *    9 kurtosis               m4 / m2^2 - 3 on central moments (the mean first, then the moments); NaN when m2 = 0
 *   10 energy_std             population standard deviation of the mean square of the frames of int(0.025 sr) samples at hop
 *                             int(0.010 sr), unpadded: 1 + (n - length) / hop of them
 *   11 speech_to_noise_ratio  speech_band_energy / (energy + 1e-10)
 *   12 rms                    sqrt(energy): the quantity silent.py compares with its threshold (the caller applies the threshold)
 *   13..15                    reserved, written as +0
 *   counts (rows, 4) int32:   [0] the total zero-crossing count, exact;  [1] speech_score = classify_speech_noise: +1 for each of
 *                             speech_band_energy > 0.001, zero_crossing_rate < 0.1, spectral_centroid < 3000, kurtosis > 5,
 *                             energy_std > 0.01, +2 for speech_to_noise_ratio > 0.6, compared in fp32, a comparison with NaN false;
 *                             [2] 1 iff the row holds a non-finite sample;  [3] the label: 1 speech (score >= 4), 0 noise, -1 non-finite
 *   frames_out (rows, F, 4) fp32, optional: per frame the centroid (Hz), the bandwidth (Hz), the roll-off BIN and the zero-crossing count.
 *   A row with a non-finite sample has columns 0..12 NaN, counts {0, 0, 1, -1} and NaN frames; no other row changes a bit.
 * Computed in fp32 (csrc/clip_features.hip): ONE launch, one workgroup per row, stateless, enqueue-only, no scratch, no atomics.  A row of
 * n <= 16384 samples is read from memory once (it is held in LDS beside the transform's workspace and the F x 128 dB table); a longer
 * row is re-read through L2.  Two neighbouring frames share one complex 2048-point transform (2^-23 of the louder one is left in the
 * other's spectrum; a frame whose windowed samples are all zero has a spectrum of exactly zero).  The band-pass runs in 256 chunks,
 * each started `warm` samples early from zero state (at sample 0 where the chunk begins before `warm`): the caller passes a warm-up
 * after which the cascade's impulse response is below 1e-7 (curate.bandpass_warmup: 512 at 16 kHz).  A row's bits depend on its samples,
 * n, sr, warm and the tables -- never on rows, the row's place in the batch or the grid; two launches give identical bits.
 * wm_clip_features_plan (host-only query, the outputs are HOST pointers, stream unused): frames = F, energy_frames = the number of
 * 25-ms frames, lds_bytes = the LDS one workgroup of the launch takes.
 * Pointers may start at any multiple of 4 bytes; inputs are borrowed.  hipErrorInvalidValue before any launch: rows, n, sample_rate or
 * warm (outside [0, 32768]) out of range, int(0.025 sr) > n, a null (frames_out excepted) or misaligned pointer, an output overlapping
 * an input or another output. */
int wm_clip_features_plan(long long rows, long long n, int sample_rate, int* frames, int* energy_frames, int* lds_bytes,
                          wm_stream_t stream);
int wm_clip_features(const float* x, const float* sos, const float* fb, const int* klo, const int* khi, const float* dct, float* feat,
                     int* counts, float* frames_out, long long rows, long long n, int sample_rate, int warm, wm_stream_t stream);

/* ---- noise suppression: a short-time spectral Wiener gate with a decision-directed a-priori SNR, and its adjoint --------------------------
 * The signal path that Ephraim-Malah / Scalart-Filho suppressors and WebRTC-style noise suppression share, as an attack on a watermark that
 * is itself a low-level noise-like signal.  A STAND-IN: one stationary noise estimate per row, no voice-activity detector, no
 * minimum-statistics tracking, no neural denoiser; a stationary tone counts as noise and is attenuated; parity with WebRTC NS, RNNoise,
 * noisereduce or any product's suppressor is unmeasured.  Defined at 16 kHz.  The output stays time-aligned with the input.
 * The gains come from a row x of n >= 1 samples and are applied to a second row src of n samples; in the forward src is x itself.
 * x, src, y are (rows, n) fp32, rows >= 1, n <= 2^34, rows * n <= 2^46; every row on its own.
 *   constants   L = 512, H = 256, K = 257 bins, M = ceil(n / H) + 1 frames; the sine window w[j] = sin(pi (j + 0.5) / L), whose square
 *               sums to 1 at 50 % overlap; eps = 1e-10; gamma_E = 0.5772156649015329
 *   framing     xp = H zeros, then the row, then zeros up to (M + 1) H samples; frame m = xp[m H : m H + L] w, so every sample lies in
 *               exactly two frames
 *   spectrum    X[m,k] = the 512-point real transform of frame m, k = 0..256;  P[m,k] = |X[m,k]|^2
 *   noise PSD   stationary, and the row judges itself:  N[k] = e^gamma_E exp((1 / M) sum_m ln(P[m,k] + eps)), the geometric mean over ALL M
 *               frames (frames of digital silence count); the factor e^gamma_E makes it unbiased on stationary Gaussian noise.  With
 *               noise_in given, a per-row (K,) profile, that is N and this pass is skipped (an attacker who knows delta's average
 *               spectrum would pass it)
 *   gain        the recursion runs over m for every k:  g[m,k] = P[m,k] / (over N[k] + eps),
 *               xi[m,k] = alpha q[m-1,k] + (1 - alpha) max(g[m,k] - 1, 0) with q[-1,k] = 1,  G[m,k] = max(xi / (1 + xi), Gmin),
 *               q[m,k] = G[m,k]^2 g[m,k];  Gmin = 10^(-reduce_db / 20), reduce_db per row: NaN becomes 0, then it is clipped to [0, 60].
 *               alpha: the decision-directed weight (0.98 is the usual one); over: the over-subtraction factor (1.0)
 *   synthesis   S[m,k] = the transform of src's frames;  yf[m] = w irfft(G[m] S[m]);  the frames are overlap-added;  y = out[H : H + n]
 * Properties: reduce_db = 0 gives Gmin = 1, so G = 1 and y = src to rounding.  With the gains held the map src -> y is self-adjoint (real
 * gains, the same window on both sides, framing is the adjoint of overlap-add), so THE BACKWARD IS THE SAME CALL: gains from the saved x,
 * src = dy.  The dependence of the gains on x is not differentiated.  An all-zero row gives exact zeros and finite gains.
 * src: null means x.  noise_in: (rows, 257) or null.  gain_out (rows, M, 257) and noise_out (rows, 257): optional.  scratch: caller-
 * allocated, contents unspecified before and after.  wm_noise_suppress_plan: host-only query (the two results are HOST pointers, stream
 * unused): frames = M, scratch_bytes = what `scratch` must hold.
 * Computed (csrc/noise_suppress.hip) in three launches: analysis in fp64 over (row, chunk of 16 frames), two frames per complex transform,
 * P to scratch as fp32 with per-chunk, per-bin sums of ln(P + eps); one thread per (row, bin) adds those sums in chunk order, forms N and runs
 * the recursion in fp64, G over P in place; synthesis in fp32 over (row, output hop), each workgroup forming the two frames that cover its
 * 256 samples, every sample of y written once.  No atomics: a row's bits depend on its samples, its reduce_db (its noise_in, alpha, over)
 * and n only, never on rows, its place in the batch or the grid; two launches give identical bits.
 * A row of x with any non-finite sample comes back all NaN in y, gain_out and noise_out; its neighbours carry the bits of a launch without
 * it.  Non-finite values in src just propagate through the arithmetic.
 * Every pointer may start at any multiple of 4 bytes; inputs are borrowed and never written.  hipErrorInvalidValue before any launch:
 * rows or n < 1, n > 2^34, rows * n > 2^46; a null x, reduce_db, y or scratch; a misaligned pointer; alpha outside [0, 1); over not finite
 * and positive; any output (y, gain_out, noise_out, scratch) overlapping an input or another output (src == x is allowed). */
int wm_noise_suppress_plan(long long rows, long long n, long long* frames, long long* scratch_bytes, wm_stream_t stream);
int wm_noise_suppress(const float* x, const float* src, const float* noise_in, const float* reduce_db, float* y,
                      float* gain_out, float* noise_out, void* scratch, long long rows, long long n,
                      float alpha, float over, wm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* WM_HIP_H */
