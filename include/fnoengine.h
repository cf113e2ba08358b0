/* fnoengine C ABI - MI355X (gfx950) FNO spectral-convolution engine.
 *
 * Drop-in boundary for the hot path of neuraloperator/pde-policylearning
 * (SURVEY.md section 8b).  The reference is pure Python/PyTorch, so "what its FFI
 * would bind" is the set of torch-op sequences below; each entry point names the
 * reference code it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - plain C: pointers, sizes, POD structs; no torch / C++ types.
 *   - every pointer is DEVICE memory owned by the caller (activations NCHW /
 *     NCDHW contiguous fp32, complex tensors interleaved (re, im) fp32) unless
 *     stated otherwise.  The library owns only immutable twiddle tables inside
 *     a plan (freed by *_plan_destroy).
 *   - all work is enqueued on the caller's hipStream_t (passed as void*), no
 *     implicit synchronisation, no allocation inside forward / backward
 *     (graph-capturable).
 *   - return 0 on success, negative FNO_E* on failure; text via fno_last_error().
 */
#ifndef FNOENGINE_H
#define FNOENGINE_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FNO_MAX_LAYERS 16
#define FNO_VERSION 100

enum { FNO_OK = 0, FNO_EINVAL = -1, FNO_EUNSUPPORTED = -2, FNO_EHIP = -3, FNO_ENOMEM = -4 };
/* torch.fft `norm=` strings */
enum { FNO_NORM_BACKWARD = 0, FNO_NORM_FORWARD = 1, FNO_NORM_ORTHO = 2 };

int fno_version(void);
const char* fno_last_error(void);
/* GEMM arithmetic of the fused model kernels.
 * 1 (default) = split precision, fp32 in / fp32 accumulate / fp32 out: every operand of a channel GEMM is scaled by a power of
 *     two taken from a published bound of its magnitude and split into TWO fp16 terms x = h + l (22 significand bits); the
 *     products h h', h l', l h' run on the fp16 matrix pipe (v_mfma_f32_32x32x16_f16: THREE products per 16-deep k block),
 *     hh and the cross terms in separate fp32 accumulators.  Where no bound is known before the operand is split (the
 *     spectral K-extension's table and spectral rows, small-K extensions, kernels of models with fewer than 1024 tiles) the
 *     operand is split into THREE bf16 terms instead and six products are kept (v_mfma_f32_32x32x16_bf16).  Error of either
 *     form against float64 = the fp32 MFMA's own (1.5e-7 relative at K = 64; DESIGN.md sections 4, 4d).
 * 0 = every GEMM on the exact fp32 matrix instruction (v_mfma_f32_32x32x2_f32).
 * Both modes cover the fused model (fno_model_*) on whole rows, the block tails (fno_model_*_tail), the fan-outs
 * (fno_fanout_*), the pointwise layers (fno_pointwise_*) and the projection heads (fno_projection_*, GELU and ReLU, every
 * output width); block stacks on loose rows (fno_model_plan_create) are split-precision only.
 * Environment FNO_GEMM_F32=1 selects 0 at load time. */
void fno_set_gemm_mode(int split_precision);
int fno_get_gemm_mode(void);
/* The mode contraction 'bixy,ioxy->boxy' (spectral_convolution.py:15-36, rno.py:51-58, basics.py:14-24) and its two
 * adjoints: 1 (default) = one real GEMM per kept mode on the fp32 matrix cores (32 / 64 channels; other channel counts
 * always take the VALU kernels); 0 = VALU kernels everywhere.  Environment FNO_MODE_GEMM_VALU=1 selects 0 at load time. */
void fno_set_mode_gemm(int mfma);
int fno_get_mode_gemm(void);

/* The spectral middle of a fused 2-D block (leading-axis DFT -> mode contraction -> leading-axis inverse DFT,
 * spectral_convolution.py:324-345): 1 (default) = one launch (k_spec_mid; 32 / 64 channels, 4 / 8 / 12 / 16 kept leading
 * modes), 0 = the three-launch sequence.  Same results to fp32 rounding.  Environment FNO_NO_FUSED_MID=1 selects 0 at
 * load time. */
void fno_set_fused_mid(int on);
int fno_get_fused_mid(void);

/* ------------------------------------------------------------------------
 * Standalone spectral convolution  y = irfftn(pad(W_c . rfftn(x)[corner_c])) (+ bias)
 * Covers the reference's three dialects:
 *   A  neuralop/models/spectral_convolution.py:303-347 (FactorizedSpectralConv, dense;
 *      modes[d] = n_modes[d] // 2, norm FORWARD via FNO default tfno.py:129, bias)
 *   B  neuralop/models/rno.py:60-77          (SpectralConv2d, modes as given, ORTHO)
 *   C  libs/models/pino_models/basics.py:79-96, 114-143 (SpectralConv2d/3d, BACKWARD;
 *      3-D: weight_last_extent = modes3, modes[2] = min(Nz/2+1, modes3))
 * Corner weights are the reference's own parameter tensors, complex64 viewed as
 * fp32 pairs, shape (Cin, Cout, modes[0], [modes[1],] weight_last_extent), in the
 * canonical corner order (lo), (hi) in 2-D and (lo,lo), (lo,hi), (hi,lo), (hi,hi)
 * over the two leading dims in 3-D.
 * One-dimensional grids (ndim = 1; neuralop FNO1d / dialect A, libs/models/pino_models/basics.py:30-58 SpectralConv1d /
 * dialect C) have ONE corner weight (Cin, Cout, weight_last_extent) and their own kernels: the truncated DFT of a whole
 * sample as a GEMM against the plan's twiddle tables, in slabs of 256 points, three launches per direction.  Limits,
 * each refused by name at plan creation: Cin, Cout in {32, 64} (they may differ); dims[0] a multiple of 128 in
 * [128, 8192]; 1 <= modes[0] <= 64 (so never the Nyquist bin); weight_planes = 0.  input_gelu is supported at every such
 * shape.  1-D arithmetic is exact fp32 in either GEMM mode: fno_set_gemm_mode does not change 1-D results.
 * ---------------------------------------------------------------------- */
typedef struct FnoSpecDesc {
  int ndim;                /* 1, 2 or 3 */
  int Cin, Cout;
  int dims[3];             /* spatial extents */
  int modes[3];            /* kept extent per corner along each dim */
  int weight_last_extent;  /* last-dim extent of the stored weights (>= modes[ndim-1]) */
  int norm;                /* FNO_NORM_* */
  int input_gelu;          /* 1: the input is a PRE-activation tensor u and the convolution acts on gelu(u) (applied while
                              the rows are staged; 2-D / 3-D: <= 64 channels, rows <= 320 floats, <= 32 kept last-dim bins).  backward
                              then returns dL/d gelu(u); the caller (fno_pointwise_backward) applies gelu'(u). */
  int weight_planes;       /* 1: the corner weights (and their gradients) are stored PLANE-MAJOR - the memory order is
                              (weight_last_extent, Cin, Cout, modes[0], [modes[1]]), i.e. the reference's tensor permuted so
                              that its last dim is outermost.  The live last-dim slices [0, modes[ndim-1]) of a dialect-C
                              weight are then one contiguous prefix (what the layout kernels, the optimizer and the gradient
                              exchange touch: PINObserverFullField at T = 1 uses 1 plane of 12).  fno_spec_backward then
                              writes the live planes of dw_corners only: the caller keeps the others zero. */
} FnoSpecDesc;

typedef struct FnoSpecPlan FnoSpecPlan;
int fno_spec_plan_create(const FnoSpecDesc* desc, FnoSpecPlan** out);
void fno_spec_plan_destroy(FnoSpecPlan* plan);
size_t fno_spec_workspace_bytes(const FnoSpecPlan* plan, int batch);
size_t fno_spec_xhat_bytes(const FnoSpecPlan* plan, int batch);
/* y = specconv(x) + bias.  xhat_save (fno_spec_xhat_bytes) receives what backward needs besides dy: the truncated
 * spectrum of x (for dW) and the mode-major transposed weights (for dx, so that backward does not re-pack them);
 * may be NULL.  fno_spec_backward with xhat = that buffer may pass w_corners = NULL. */
int fno_spec_forward(const FnoSpecPlan* plan, int batch, const float* x, const float* const* w_corners,
                     const float* bias /*nullable (Cout)*/, float* y, float* xhat_save, void* ws, size_t ws_bytes,
                     void* stream);
/* autograd of the above: any of dx / dw_corners / dbias may be NULL. */
int fno_spec_backward(const FnoSpecPlan* plan, int batch, const float* dy, const float* xhat_save,
                      const float* const* w_corners, float* dx, float* const* dw_corners, float* dbias, void* ws,
                      size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Whole-model fused path: neuralop.models.FNO on its default configuration
 * (tfno.py:195-211: Lifting :11-20 -> n_layers x FNOBlocks.forward fno_block.py:123-170
 * with fno_skip='linear', GELU gate `index < n_layers - index` :149 -> Projection :23-38).
 * One fused kernel per block (skip 1x1 conv + last-dim inverse DFT + bias + gated GELU +
 * last-dim forward DFT of the next block), activations stored pre-activation.
 * Grids: hidden width 32 or 64; rows (last dim) of 32 / 64 / 128 / 256 tile the kernels' 128- or 256-pixel tiles and take the
 * row transforms as kernel epilogues; any other last dim in 32..320 on planes that are a multiple of 128 pixels (96 x 96,
 * 160 x 160, the PINO observers' padded time axis 73, ...) runs in "loose rows" mode: 128-pixel tiles of the flattened plane,
 * spectral rows gathered per tile, last-dim forward transforms as separate passes (split-precision GEMM mode only).
 * fno_model_plan_create returns FNO_EUNSUPPORTED for everything else; callers then compose fno_spec_* / fno_pointwise_*.
 * ---------------------------------------------------------------------- */
typedef struct FnoModelDesc {
  int ndim;            /* 2 or 3 */
  int Cin, C, Cout;    /* lifting in, hidden width, projection out */
  int hidden_proj;     /* projection_channels (256) */
  int n_layers;
  int dims[3];
  int modes[3];        /* kept per corner per dim = n_modes[d] // 2 (spectral_convolution.py:202-203) */
  int norm;            /* FNO_NORM_* (FNO default: FORWARD) */
  unsigned gelu_mask;  /* bit l set <=> GELU after block l (fno_block.py:149) */
  int weight_planes;   /* 1: spec_w tensors (and their gradients) are stored plane-major, see FnoSpecDesc */
} FnoModelDesc;

typedef struct FnoModelParams {       /* all fp32 device pointers, reference parameter layouts */
  const float* lift_w;                /* lifting.fc.weight (C, Cin, 1..)  */
  const float* lift_b;                /* lifting.fc.bias (C)              */
  const float* skip_w[FNO_MAX_LAYERS];      /* fno_blocks.fno_skips.l.weight (C, C, 1..) */
  const float* spec_w[FNO_MAX_LAYERS][4];   /* fno_blocks.convs.weight[2^(d-1) l + corner] (C, C, m.., 2) */
  const float* spec_bias;             /* fno_blocks.convs.bias (L, C, 1..) or NULL */
  const float* proj_w1;               /* projection.fc1.weight (hidden_proj, C, 1..) */
  const float* proj_b1;
  const float* proj_w2;               /* projection.fc2.weight (Cout, hidden_proj, 1..) */
  const float* proj_b2;
} FnoModelParams;

typedef struct FnoModelGrads {        /* same shapes as the parameters; written, not accumulated */
  float* lift_w;
  float* lift_b;
  float* skip_w[FNO_MAX_LAYERS];
  float* spec_w[FNO_MAX_LAYERS][4];
  float* spec_bias;
  float* proj_w1;
  float* proj_b1;
  float* proj_w2;
  float* proj_b2;
} FnoModelGrads;

typedef struct FnoModelPlan FnoModelPlan;
int fno_model_plan_create(const FnoModelDesc* desc, FnoModelPlan** out);
void fno_model_plan_destroy(FnoModelPlan* plan);
size_t fno_model_workspace_bytes(const FnoModelPlan* plan, int batch);
/* bytes of the forward->backward stash: (n_layers+1) pre-activation tensors +
 * n_layers truncated spectra */
size_t fno_model_saved_bytes(const FnoModelPlan* plan, int batch);
int fno_model_forward(const FnoModelPlan* plan, int batch, const FnoModelParams* p, const float* x, float* y,
                      void* saved /*nullable: inference*/, void* ws, size_t ws_bytes, void* stream);
int fno_model_backward(const FnoModelPlan* plan, int batch, const FnoModelParams* p, const float* x,
                       const float* dy, const void* saved, const FnoModelGrads* g, void* ws, size_t ws_bytes,
                       void* stream);
/* Block stacks.  FnoModelDesc.Cin == 0 drops the lifting (x is the (B, C, ...) input of block 0) and
 * Cout == 0 drops the projection (y = u_L, (B, C, ...); the last block must then carry no GELU).  This is
 * the fused form of the reference's other "Fourier layers":
 *   neuralop/models/rno.py:215-228  FourierLayer2d = SpectralConv2d(ortho) + Conv1d(k=1)   (n_layers = 1)
 *   libs/models/pino_models/pinobserver.py:221-226  sp_convs[i](x) + ws[i](x), GELU except last
 * with skip_w[l] = the Conv1d weight and spec_bias = the Conv1d biases (L, C).  For such stacks the
 * input gradient dx (B, C, ...) is produced as well (NULL to skip). */
int fno_model_backward_dx(const FnoModelPlan* plan, int batch, const FnoModelParams* p, const float* x,
                          const float* dy, const void* saved, const FnoModelGrads* g, float* dx, void* ws,
                          size_t ws_bytes, void* stream);
/* One-layer block stacks with a tail: the layers of the RNO regressor, neuralop/models/rno.py:92-106
 * SpectralConvWithFC.forward = act(spec_conv(dropout(x)) + Linear(x)) with act = ReLU (rno.py:214-215), channels-first.
 *   forward   y = max(u, 0) if relu_out else u,   u = specconv(drop(x)) + skip_w x + bias
 *   backward  g = dy * (y > 0) (the mask is read off the forward's output `y`), dx = skip_w^T g + drop-scale * (spectral
 *             adjoint of g); parameter gradients as fno_model_backward_dx
 * drop(x)[e] = x[e] * s[e], s[e] = 0 with probability drop_p and 1 / (1 - drop_p) otherwise, decided by a hash of the
 * element index and the two 32-bit words at `drop_seed` (device memory; the caller draws them per call and passes the same
 * pointer to the backward, which regenerates s instead of reading a mask; fno_dropout_scale writes s out for tests).
 * drop_p = 0 disables the dropout (evaluation mode).  Plans: Cin = Cout = 0, n_layers = 1, 32 / 64 channels, rows of
 * 32 / 64 / 128 floats, either GEMM mode; anything else returns FNO_EUNSUPPORTED. */
typedef struct FnoBlockTail {
  int relu_out;
  float drop_p;
  const unsigned* drop_seed;   /* device pointer to 2 x uint32, or NULL when drop_p == 0 */
  const float* y;              /* backward only: the forward's output (B, C, ...) */
} FnoBlockTail;
int fno_model_forward_tail(const FnoModelPlan* plan, int batch, const FnoModelParams* p, const float* x, float* y,
                           void* saved, void* ws, size_t ws_bytes, void* stream, const FnoBlockTail* tail);
int fno_model_backward_tail(const FnoModelPlan* plan, int batch, const FnoModelParams* p, const float* x,
                            const float* dy, const void* saved, const FnoModelGrads* g, float* dx, void* ws,
                            size_t ws_bytes, void* stream, const FnoBlockTail* tail);
int fno_dropout_scale(size_t n, float drop_p, const unsigned* seed /*device, 2 words*/, float* out /*device, n*/, void* stream);

/* The same pass in parts: layers l_hi .. l_lo (descending; l_hi = n_layers-1 includes the projection, l_lo = 0 the
 * lifting).  Calls over a partition of the layers with the SAME workspace reproduce the full pass bit for bit, and each
 * call finishes the gradients of its own layers - a data-parallel caller starts the all-reduce of the late layers'
 * gradients while the early layers are still being differentiated (trainer.FlatGradBucket.for_fno). */
int fno_model_backward_part(const FnoModelPlan* plan, int batch, const FnoModelParams* p, const float* x,
                            const float* dy, const void* saved, const FnoModelGrads* g, float* dx, void* ws,
                            size_t ws_bytes, void* stream, int l_hi, int l_lo);

/* Fan-out of Fourier layers over ONE input: y_j = SpecConv_j(x) + W_j x + b_j, j < n_out.  The GRU-style cell of the
 * recurrent neural operator evaluates eight Fourier layers on three distinct inputs (neuralop/models/rno.py:254-260:
 * f1, f3, f5, f7 on x; f2, f4, f8 on h; f6 on r * h); the reference transforms each input once per layer.  Here the
 * forward transforms of the shared input run once for all members, and backward produces dx = sum_j dL/dx|_j by chaining
 * the members through the block kernel's gradient-addend input (no accumulation pass, no n_out separate dx tensors).
 * `plan` is a block-stack plan (Cin = Cout = 0, gelu_mask = 0) created with n_layers >= n_out; members occupy layer slots
 * 0..n_out-1 of FnoModelParams / FnoModelGrads (skip_w, spec_w only), biases are separate (C) arrays (entries / the
 * array itself nullable).  The members' mode contractions and leading-axis passes run as ONE launch each (member-major
 * buffers, member index on the contraction grid).  Workspace: fno_fanout_workspace_bytes; stash: fno_fanout_saved_bytes. */
size_t fno_fanout_saved_bytes(const FnoModelPlan* plan, int batch, int n_out);
size_t fno_fanout_workspace_bytes(const FnoModelPlan* plan, int batch, int n_out);
int fno_fanout_forward(const FnoModelPlan* plan, int batch, int n_out, const FnoModelParams* p, const float* const* bias,
                       const float* x, float* const* y, void* saved, void* ws, size_t ws_bytes, void* stream);
int fno_fanout_backward(const FnoModelPlan* plan, int batch, int n_out, const FnoModelParams* p, const float* x,
                        const float* const* dy, const void* saved, const FnoModelGrads* g, float* const* dbias, float* dx,
                        void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Training-step tail (run_pde_observers.py:185-193), SURVEY.md section 8(f) rank 2.
 * Loss: pd = pred*(std+eps)+mean, td = target*(std+eps)+mean  (NormalizerGivenMeanStd.cuda_decode,
 * libs/utilities3.py:115-129; mean/std NULL = identity; stat_len = 1 or n, broadcast over the batch),
 * loss = sum_b ||pd_b - td_b||_2 / ||td_b||_2, divided by batch when size_average
 * (LpLoss.rel, libs/utilities3.py:323-334).  forward leaves per-sample coefficients in `ws`
 * (fno_lploss_workspace_bytes) for backward, which writes dloss/dpred scaled by the device scalar
 * *grad_loss (NULL = 1).  No host synchronisation (the reference's loss.item() is the caller's choice).
 * ---------------------------------------------------------------------- */
size_t fno_lploss_workspace_bytes(int batch);
int fno_lploss_rel_forward(int batch, size_t n_per_sample, const float* pred, const float* target, const float* mean,
                           const float* std, int stat_len, float eps, int size_average, float* loss /*device scalar*/,
                           void* ws, size_t ws_bytes, void* stream);
int fno_lploss_rel_backward(int batch, size_t n_per_sample, const float* pred, const float* target, const float* std,
                            int stat_len, float eps, const float* grad_loss, float* dpred, const void* ws,
                            size_t ws_bytes, void* stream);
/* torch.optim.Adam (run_pde_observers.py:134: lr, weight_decay as L2 added to the gradient; no amsgrad)
 * on ONE flat fp32 bucket of n elements: param / grad / exp_avg / exp_avg_sq, 16-byte aligned.
 * `step` is the 1-based step count.  The hyperparameters are DOUBLES, as torch.optim.Adam holds them: step size, bias
 * corrections and the (1 - beta) weights are formed in double and rounded once, as torch's scalar arguments are
 * (1.0f - 0.999f is 1.3e-5 away from the 0.001 torch hands to addcmul_). */
int fno_adam_step(size_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, double lr, double beta1,
                  double beta2, double eps, double weight_decay, int step, void* stream);
/* Same update with the step count on the DEVICE: *step_counter is incremented and the bias corrections are
 * derived from it by a one-thread kernel, so a captured hipGraph of the whole training step can be
 * replayed (no host-side scalar changes between replays).  scratch2: two device floats. */
int fno_adam_step_dev(size_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, double lr, double beta1,
                      double beta2, double eps, double weight_decay, int* step_counter, float* scratch2, void* stream);
/* The same update for a bucket that holds dialect-C spectral weights of which only the last-dim slice [..., :k] ever sees
 * data (libs/models/pino_models/basics.py:119-139 cuts the spectrum at min(Nz/2+1, modes3): PINObserverFullField at T = 1
 * uses 1/12 of its 906 MB).  The gradient of the rest is exactly zero, so what torch.optim.Adam (run_pde_observers.py:134)
 * does to such an element is a recurrence on (p, m, v) alone - g = weight_decay * p.  It is skipped per step and REPLAYED in
 * one pass when the slice is needed; results are bit-identical to stepping it every time.
 *   A sliced block is rows x row_len floats, the first live_len floats of each row live (both even: complex pairs);
 *   a plane-major weight (FnoSpecDesc.weight_planes) is ONE row whose live planes are its head.
 *   fno_adam_step_range: fno_adam_step on a sub-range; `dyn` (device, 2 floats: fno_adam_prep_dev) replaces `step`.
 *   fno_adam_prep_dev:   ++*step_counter and the step's two scalars into scratch2 (graph-replayable, once per step).
 *   fno_adam_step_live:  the live part of a block; param / grad in the full layout, moments compact (rows x live_len).
 *   fno_adam_scalars:    host: {lr / (1 - beta1^step), sqrt(1 - beta2^step)} exactly as fno_adam_step derives them.
 *   fno_adam_replay_prep: the same two scalars for steps step_from .. step_from + nsteps - 1 on the device
 *                        (scal: 2 * nsteps floats), as fno_adam_step_dev derives them.
 *   fno_adam_replay_dead: takes the dead part of a block through the nsteps steps described by `scal`; dead moments
 *                        compact (rows x (row_len - live_len)), read unless moments_zero, always written. */
void fno_adam_scalars(double lr, double beta1, double beta2, int step, float* out2);
int fno_adam_prep_dev(int* step_counter, float* scratch2, double lr, double beta1, double beta2, void* stream);
int fno_adam_step_range(size_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, double lr, double beta1,
                        double beta2, double eps, double weight_decay, int step, const float* dyn, void* stream);
int fno_adam_step_live(size_t rows, int row_len, int live_len, float* param, const float* grad, float* exp_avg_live,
                       float* exp_avg_sq_live, double lr, double beta1, double beta2, double eps, double weight_decay, int step,
                       const float* dyn, void* stream);
int fno_adam_replay_prep(float* scal, int step_from, int nsteps, double lr, double beta1, double beta2, void* stream);
int fno_adam_replay_dead(size_t rows, int row_len, int live_len, float* param, float* dead_exp_avg, float* dead_exp_avg_sq,
                         int moments_zero, const float* scal, int nsteps, double beta1, double beta2, double eps,
                         double weight_decay, void* stream);

/* ------------------------------------------------------------------------
 * PINO residual loss, SURVEY.md section 8(f) rank 1: FDM_NS_vorticity + Channelflow_PINO_loss
 * (libs/envs/diff_control_env.py:5-60 == libs/pino_utils/losses.py:68-104, 246-262; train_pino.py:98-101).
 *   u (B, n, n, nt) model output, u0 (B, n, n) initial vorticity, forcing (n, n), visc (B) = 1 / Re,
 *   Du = w_t + u . grad(w) - visc lap(w) with spectral derivatives over (x, y) and a central difference in t
 *   on the interior time levels; loss_f = mean_b ||Du_b - forcing|| / ||forcing||, loss_ic = mean_b
 *   ||u_b(t = 0) - u0_b|| / ||u0_b||  (LpLoss(size_average=True).rel).
 * forward leaves the derived fields and per-sample coefficients in `ws` (fno_pino_loss_workspace_bytes);
 * backward writes du = g_ic * dloss_ic/du + g_f * dloss_f/du (device scalars, NULL = 1).
 * n must be 32, 64, 128 (one plane per workgroup, in-LDS radix-2 FFTs) or 256 (three slab passes each way, planes in
 * chunks of 64: csrc/k_pino_loss2.h).
 * ---------------------------------------------------------------------- */
size_t fno_pino_loss_workspace_bytes(int batch, int n, int nt);
int fno_pino_loss_forward(int batch, int n, int nt, const float* u, const float* u0, const float* forcing,
                          const float* visc, float t_interval, float* loss_ic, float* loss_f, void* ws, size_t ws_bytes,
                          void* stream);
int fno_pino_loss_backward(int batch, int n, int nt, const float* u, const float* u0, const float* forcing,
                           const float* visc, float t_interval, const float* g_ic, const float* g_f, float* du, void* ws,
                           size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Burgers residual loss of the PINO models: FDM_Burgers + PINO_loss (libs/pino_utils/losses.py:200-243; the loss of
 * train_2d_burger, libs/pino_utils/train_2d.py:119-194).
 *   u (B, nt, nx) model output with x contiguous, u0 (B, nx) initial condition, visc a host scalar, domain length 1,
 *   dt = 1 / (nt - 1);  Du[b, j] = (u[b, j+1] - u[b, j-1]) / (2 dt) + ux u - visc uxx on the rows j = 1 .. nt - 2,
 *   ux / uxx the spectral derivatives along x (no Nyquist term in ux, -(pi nx)^2 in uxx);
 *   loss_f = mean Du^2, loss_u = mean (u[:, 0] - u0)^2 (F.mse_loss), both float64 sums in a fixed order.
 * forward leaves Du (B, nt - 2, nx) first in `ws`, then ux and the partial sums (fno_burgers_loss_workspace_bytes);
 * backward reads them and writes du = g_u * dloss_u/du + g_f * dloss_f/du (device scalars, NULL = 1) into all of (B, nt, nx).
 * nx must be 32, 64 or 128 (FNO_EUNSUPPORTED otherwise; odd nx, nt < 3 and batch < 1 are FNO_EINVAL); the checks need no GPU.
 * ---------------------------------------------------------------------- */
size_t fno_burgers_loss_workspace_bytes(int batch, int nt, int nx);
int fno_burgers_loss_forward(int batch, int nt, int nx, const float* u, const float* u0, float visc, float* loss_u,
                             float* loss_f, void* ws, size_t ws_bytes, void* stream);
int fno_burgers_loss_backward(int batch, int nt, int nx, const float* u, const float* u0, float visc, const float* g_u,
                              const float* g_f, float* du, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Darcy residual loss of the PINO models: FDM_Darcy + darcy_loss (libs/pino_utils/losses.py:6-65) with the mollifier and
 * the relative-L2 data term of train_2d_operator (libs/pino_utils/train_2d.py:58-82) in the same launches.
 *   out, a, y (B, S, S) with the first grid index x, h = 1 / (S - 1);  pred = out * mol, mol (S, S) or NULL (pred = out);
 *   Du[b, p, q] = -( a[p+1,q] (pred[p+2,q] - pred[p,q]) - a[p-1,q] (pred[p,q] - pred[p-2,q])
 *                  + a[p,q+1] (pred[p,q+2] - pred[p,q]) - a[p,q-1] (pred[p,q] - pred[p,q-2]) ) / (4 h^2),  p, q = 2 .. S-3;
 *   loss_f = mean_b ||Du_b - 1||_2 / (S - 4);  loss_data = mean_b ||pred_b - y_b||_2 / ||y_b||_2, only with y (y and
 *   loss_data are given together or both NULL, FNO_EINVAL otherwise).  Sums are float64 in a fixed order.
 * forward leaves Du (B, S - 4, S - 4) first in `ws`, then the partial sums and the per-sample norms
 * (fno_darcy_loss_workspace_bytes); backward reads them and writes dout = g_data * dloss_data/dout + g_f * dloss_f/dout
 * (device scalars, NULL = 1; `a` is data and gets no gradient) into all of (B, S, S).  A sample whose residual norm is
 * exactly zero contributes a zero gradient (the reference's 0 / 0 is NaN there).
 * Every S from 5 to 4096: S < 5 and batch < 1 are FNO_EINVAL, S > 4096 FNO_EUNSUPPORTED; the checks need no GPU.
 * ---------------------------------------------------------------------- */
size_t fno_darcy_loss_workspace_bytes(int batch, int S);
int fno_darcy_loss_forward(int batch, int S, const float* out, const float* mol, const float* a, const float* y,
                           float* loss_data, float* loss_f, void* ws, size_t ws_bytes, void* stream);
int fno_darcy_loss_backward(int batch, int S, const float* out, const float* mol, const float* a, const float* y,
                            const float* g_data, const float* g_f, float* dout, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Sobolev (H1) and L2 training losses of neuralop: LpLoss (p = 2) and H1Loss, neuralop/training/losses.py:62-277.
 *   x, y (planes, dims[0] .. dims[d-1]) fp32 contiguous, d = 1, 2 or 3 grid axes, a plane = one (batch, channel) index;
 *   e = x - y;  D_k v[i] = (v[i+1] - v[i-1]) / (2 h_k) with indices mod dims[k] (torch.roll); where bit k of fix_mask is set
 *   (fix_x_bnd is bit 0) rows 0 and dims[k]-1 are (v[1] - v[0]) / h_k and (v[n-1] - v[n-2]) / h_k instead;
 *   num = sum e^2 + [order 1] sum_k sum (D_k e)^2,  den = the same of y, per plane, float64 in a fixed order;
 *   value[plane] = relative ? sqrt(num / den) : sqrt(vol * num), vol = prod h_k  (order 0 is LpLoss, order 1 H1Loss).
 * The host passes inv2h[k] = 1 / (2 h_k), invh[k] = 1 / h_k (HOST arrays of d doubles, like dims) and vol, all float64.
 * batch_reduce 0: none.  1 / 2: the planes are a (planes / channels, channels) layout and reduced[c] is the sum / mean of
 * value[b, c] over b in a fixed order (`reduced` (channels) is required then and `channels` must divide planes).
 * forward leaves the per-workgroup partial sums and (num, den) per plane in `ws` (fno_sobolev_loss_workspace_bytes; float64
 * data only); backward reads (num, den) and writes dx = s (e + sum_k D_k^T D_k e) into all of x's extent, s = g / sqrt(num den)
 * or g sqrt(vol) / sqrt(num), g = grad[plane] without a batch reduction, grad[plane % channels] (times 1 / batch for the
 * mean) with one.  A plane whose num is exactly zero gets a zero gradient (the reference's autograd gives NaN there); the
 * forward value follows IEEE (den = 0: inf or NaN).  y is data and gets no gradient.
 * FNO_EINVAL: d outside 1..3, an extent < 2, planes < 1, order / relative outside 0..1, fix_mask outside d bits, an unknown
 * batch_reduce, channels not dividing planes, a null required pointer, a short workspace.  FNO_EUNSUPPORTED: a plane of 2^31
 * elements or more.  All of it is decided before anything is launched and needs no GPU; workspace_bytes returns 0 there.
 * ---------------------------------------------------------------------- */
size_t fno_sobolev_loss_workspace_bytes(int planes, int d, const int* dims, int order);
int fno_sobolev_loss_forward(int planes, int channels, int d, const int* dims, int order, int relative, int fix_mask,
                             int batch_reduce, const double* inv2h, const double* invh, double vol, const float* x,
                             const float* y, float* value, float* reduced, void* ws, size_t ws_bytes, void* stream);
int fno_sobolev_loss_backward(int planes, int channels, int d, const int* dims, int order, int relative, int fix_mask,
                              int batch_reduce, const double* inv2h, const double* invh, double vol, const float* x,
                              const float* y, const float* grad, float* dx, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Spectral Sobolev loss of the original FNO code base: HsLoss, libs/utilities3.py:339-405.
 *   x, y (batch, nx, ny, channels) fp32 contiguous, channels LAST; e = x - y, E = fft2(e), Y = fft2(y) per (sample, channel)
 *   plane; r2 = kx^2 + ky^2 of the absolute wave numbers |k|, k = [0 .. n/2-1, -n/2 .. -1] (the Nyquist index carries n/2);
 *   num_j = w2[j] sum_{kx,ky,c} r2^j |E|^2,  den_j = w2[j] sum r2^j |Y|^2,  j < terms (w2: a HOST array of `terms` doubles,
 *   the squared coefficients 1, a[0]^2, a[1]^2 of |k|^0, |k|^2, |k|^4), float32 per bin, float64 sums in a fixed order;
 *   group 0: value[b] = sqrt(sum_j num_j) / sqrt(sum_j den_j);  group 1: value[b] = (sum_j sqrt(num_j) / sqrt(den_j)) / divisor
 *   (the reference divides by k + 1 whatever the number of terms; `divisor` is read with group 1 only).
 * reduce 0: none.  1 / 2: reduced[0] is the sum / mean of value[b] over b in a fixed order (`reduced` is required then).
 * forward leaves the per-workgroup sums and (num_j, den_j) per sample in `ws` (fno_hs_loss_workspace_bytes; float64 data only);
 * backward reads them and writes dx = d(sum_b g_b value[b]) / dx into all of x's extent, g_b = grad[b] without a reduction,
 * grad[0] (times 1 / batch for the mean) with one.  A term whose num_j is exactly zero (group 0: a sample whose sum is)
 * contributes a zero gradient (the reference's autograd gives NaN there); the forward value follows IEEE (den = 0: inf or NaN).
 * y is data and gets no gradient.
 * FNO_EINVAL: nx != ny or outside {32, 64, 128}, batch or channels < 1, terms outside 1..3, group outside 0..1, a grouped
 * divisor that is not positive, an unknown reduce, a null required pointer, a short workspace.  FNO_EUNSUPPORTED: batch times
 * ceil(channels / 2) workgroups beyond the grid limit of 2^31 - 1.  All of it is decided before anything is launched and needs
 * no GPU; workspace_bytes returns 0 for batch or channels < 1 and beyond that limit.
 * ---------------------------------------------------------------------- */
size_t fno_hs_loss_workspace_bytes(int batch, int channels);
int fno_hs_loss_forward(int batch, int nx, int ny, int channels, int terms, const double* w2, int group, double divisor,
                        int reduce, const float* x, const float* y, float* value, float* reduced, void* ws, size_t ws_bytes,
                        void* stream);
int fno_hs_loss_backward(int batch, int nx, int ny, int channels, int terms, const double* w2, int group, double divisor,
                         int reduce, const float* x, const float* y, const float* grad, float* dx, void* ws, size_t ws_bytes,
                         void* stream);

/* ------------------------------------------------------------------------
 * Gates of the recurrent neural operator cell, neuralop/models/rno.py:254-260 (all tensors (B, C, X, Y) fp32,
 * n elements, 16-byte aligned, n % 4 == 0; b* are the cell's SCALAR biases on the device):
 *   reset gate : r = sigmoid(a3 + a4 + b2), rh = r * h                                   (:256-257)
 *   output gate: z = sigmoid(a1 + a2 + b1), z2 = sigmoid(a7 + a8 + b4), s3 = a5 + a6 + b3,
 *                h_new = (1 - z) * h + z2 * selu(s3)                                     (:254-255, :257-260)
 * a_i = f_i(.) are the cell's Fourier layers.  backward returns the gradient of each pre-activation sum
 * (shared by its two addends), the direct gradient to h, and fno_rno_gate_partials() per-workgroup partial
 * sums of every bias gradient (reset: [P]; output: [3][P] for b1, b4, b3), accumulated and stored in DOUBLE
 * (tens of millions of terms of either sign per scalar), to be summed by the caller.
 * ---------------------------------------------------------------------- */
int fno_rno_gate_partials(void);
int fno_rno_reset_gate_forward(size_t n, const float* a3, const float* a4, const float* b2, const float* h, float* r,
                               float* rh, void* stream);
int fno_rno_reset_gate_backward(size_t n, const float* d_rh, const float* r, const float* h, float* d_s, float* d_h,
                                double* db_partials, void* stream);
int fno_rno_output_gate_forward(size_t n, const float* a1, const float* a2, const float* b1, const float* a7,
                                const float* a8, const float* b4, const float* a5, const float* a6, const float* b3,
                                const float* h, float* z, float* z2, float* s3, float* h_new, void* stream);
int fno_rno_output_gate_backward(size_t n, const float* g, const float* z, const float* z2, const float* s3,
                                 const float* h, float* d_s1, float* d_s7, float* d_s3, float* d_h, double* db_partials,
                                 void* stream);

/* ------------------------------------------------------------------------
 * Pointwise channel mix  y[b, o, p] = sum_i w[o, i] x[b, i, p] + bias[o] + addend[b, o, p]  and its autograd:
 * the Conv1d(k=1) beside every spectral convolution of the observer models
 * (libs/models/pino_models/pinobserver.py:221-226 `sp_convs[i](x) + ws[i](x)`; neuralop/models/rno.py:224-228),
 * for grids the fused block stacks do not cover (odd last dimension).  x, y, addend, dy, dx: (B, C, PW) fp32,
 * C in {32, 64}, PW % 128 == 0; w (C, C) row-major [o][i]; bias / addend / dx_addend / dx / dbias nullable.
 * The gradient w.r.t. `addend` is dy itself.
 * input_gelu = 1: x is a PRE-activation tensor and the mix acts on gelu(x) (the previous layer's activation applied on
 * load, as in the fused block stack); backward then returns dx = (W^T dy + dx_addend) * gelu'(x), where dx_addend is
 * the gradient arriving at gelu(x) from its other consumer (the spectral convolution beside the mix): one layer of
 * `act(sp_conv(x) + w(x))` chains (pinobserver.py:221-226) costs no separate activation or accumulation pass.
 * ---------------------------------------------------------------------- */
size_t fno_pointwise_workspace_bytes(int channels);
int fno_pointwise_forward(int batch, int channels, size_t plane, const float* x, const float* w, const float* bias,
                          const float* addend, int input_gelu, float* y, void* stream);
int fno_pointwise_backward(int batch, int channels, size_t plane, const float* x, const float* w, const float* dy,
                           const float* dx_addend, int input_gelu, float* dx, float* dw, float* dbias, void* ws,
                           size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Projection head on its own:  y = W2 gelu(W1 x + b1) + b2, x (B, C, PW), C in {32, 64}, hidden 128 or 256,
 * Cout = 1, PW % 128 == 0: the `fc1 -> act -> fc2` tail of the observer models
 * (libs/models/pino_models/pinobserver.py:231-233, 270-273; neuralop/models/tfno.py:23-38), with the FNO
 * projection kernels (hidden tensor never materialised; backward recomputes it).  w1 (hidden, C), w2 (1, hidden).
 * backward writes dx and all four parameter gradients.  Either GEMM mode (fno_set_gemm_mode).
 * ---------------------------------------------------------------------- */
size_t fno_projection_workspace_bytes(int channels, int hidden);
int fno_projection_forward(int batch, int channels, int hidden, int cout, size_t plane, const float* x, const float* w1,
                           const float* b1, const float* w2, const float* b2, float* y, void* stream);
int fno_projection_backward(int batch, int channels, int hidden, int cout, size_t plane, const float* x,
                            const float* w1, const float* b1, const float* w2, const float* dy, float* dx, float* dw1,
                            float* db1, float* dw2, float* db2, void* ws, size_t ws_bytes, void* stream);
/* The same head with the hidden activation chosen by the caller: FNO_ACT_GELU (the two calls above) or FNO_ACT_RELU,
 * the `Linear(freq_dim, 4 freq_dim) -> ReLU -> Linear(4 freq_dim, 1)` regressor that ends RNO2d
 * (neuralop/models/rno.py:171-175, built with activation='relu' at :319-320; hidden width 256 only). */
#define FNO_ACT_GELU 0
#define FNO_ACT_RELU 1
int fno_projection_forward_act(int batch, int channels, int hidden, int cout, size_t plane, const float* x,
                               const float* w1, const float* b1, const float* w2, const float* b2, int hidden_act,
                               float* y, void* stream);
int fno_projection_backward_act(int batch, int channels, int hidden, int cout, size_t plane, const float* x,
                                const float* w1, const float* b1, const float* w2, const float* dy, int hidden_act,
                                float* dx, float* dw1, float* db1, float* dw2, float* db2, void* ws, size_t ws_bytes,
                                void* stream);

/* ------------------------------------------------------------------------
 * Channel MLP of an FNO block built with use_mlp=True (neuralop/models/fno_block.py:123-170, mlp.py:26-54,
 * skip_connections.py:38-74), one fused kernel per direction:
 *     y = [gelu]( gelu(W2 gelu(W1 u + b1) + b2) + gate (.) x )
 * u (B, C, PW): the Fourier part's (activated) output, x (B, C, PW): the block's input, w1 (hidden, C), w2 (C, hidden),
 * gate (C): the soft-gating weight, or null for the identity skip; gelu_out: GELU on the sum (every block but the last).
 * (C, hidden) in {(64, 32), (64, 64), (32, 32)}, PW % 128 == 0; anything else is an error code and launches nothing.
 * backward recomputes every intermediate from u and x and writes du, dx (null: not wanted) and the parameter
 * gradients (dgate null iff gate is null); partial sums go through the workspace and a fixed-order reduction, so results are
 * bitwise repeatable.  The GEMMs are exact fp32 in either GEMM mode (fno_set_gemm_mode).
 * ---------------------------------------------------------------------- */
size_t fno_channel_mlp_workspace_bytes(int channels, int hidden, int batch, size_t plane);
int fno_channel_mlp_forward(int batch, int channels, int hidden, size_t plane, const float* u, const float* x,
                            const float* w1, const float* b1, const float* w2, const float* b2, const float* gate,
                            int gelu_out, float* y, void* stream);
int fno_channel_mlp_backward(int batch, int channels, int hidden, size_t plane, const float* u, const float* x,
                             const float* w1, const float* b1, const float* w2, const float* b2, const float* gate,
                             int gelu_out, const float* dy, float* du, float* dx, float* dw1, float* db1, float* dw2,
                             float* db2, float* dgate, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Domain padding of the FNO family (neuralop/models/padding.py:35-95; tfno.py:195-211 pads the lifted field, runs the
 * Fourier blocks on the extended grid and crops before the projection).  x (planes, dims[0..ndim)) fp32 with planes =
 * batch * channels, y (planes, dims[d] + before[d] + after[d]); ndim 1, 2 or 3.  dims / before / after are HOST arrays of
 * ndim ints, read before the call returns.
 *   fno_domain_pad:  y = x with before[d] zeros in front of and after[d] zeros behind axis d.  Every element of y is written;
 *     the margin is +0.0f, the interior is copied bit for bit (NaN payloads, infinities, -0.0).
 *   fno_domain_crop: x = the interior of y.
 * Each is the other's adjoint: the backward of a pad is the crop of the gradient and the reverse.  All pads zero is a plain
 * copy.  One launch, no workspace, no atomics; stores are whole 16-byte vectors wherever the output's address allows it
 * (tensors need 4-byte alignment only).  FNO_EINVAL: a null pointer, ndim outside 1..3, a dimension < 1, a negative pad;
 * FNO_EUNSUPPORTED: more than 2^30 elements along a padded axis or more than 2^62 in the padded tensor.  The checks need
 * no GPU.
 * ---------------------------------------------------------------------- */
int fno_domain_pad(int ndim, size_t planes, const int* dims, const int* before, const int* after, const float* x, float* y,
                   void* stream);
int fno_domain_crop(int ndim, size_t planes, const int* dims, const int* before, const int* after, const float* y, float* x,
                    void* stream);

/* ------------------------------------------------------------------------
 * Device-resident training data (libs/pde_data_loader.py DeviceBatches): a batch assembled from raw snapshots that stay on the
 * device.  src is a pool of n_src snapshots of snap_elems elements each, float32 (src_dtype 0) or float64 (1), the codes of
 * fno_chanflow_rhs; idx (count) int64 on the device picks the entries.  For entry e, i < rows, j < cols:
 *     x = src[idx[e] * snap_elems + offset + i * row_stride + j * col_stride]
 *     out[e * out_stride + i * cols + j] = (float)((x - mean[i][j]) / (std_[i][j] + eps))
 * mean, std_ (rows, cols) contiguous of stat_dtype (same codes).  The arithmetic type is the host's promotion of
 * NormalizerGivenMeanStd.encode: float64 if either dtype is float64, float32 if both are float32; std_ + eps is formed in the
 * statistics' type (eps rounded to float32 first there, as tensor + python_float does); every operation is rounded once with
 * a true division, and one last rounding gives the float32.  mean and std_ both NULL: out = (float)x, a gather and cast
 * (stat_dtype is not read).  The one view covers downsample + crop (row_stride = d * C0, col_stride = d), a plane V[:, p, :]
 * (offset = p * Nz, row_stride = Ny * Nz), a whole field as a 2-D array, and one plane of a (T, P, X, Z) target (out advanced by
 * p * X * Z, out_stride = P * X * Z).
 * Every index is compared unsigned against n_src before it becomes an address: an entry whose index is out of range reads
 * nothing and its rows * cols outputs are NaN.  One launch, no workspace, no atomics, 64-bit addressing; stores are whole
 * 16-byte vectors wherever the output's address allows it (tensors need the alignment of their element only).
 * FNO_EINVAL: a null src / idx / out, exactly one of mean / std_, an unknown dtype, rows or cols < 1, out_stride < rows * cols,
 * offset + (rows - 1) * row_stride + (cols - 1) * col_stride >= snap_elems, a misaligned tensor; FNO_EUNSUPPORTED: a pool
 * beyond 2^62 bytes or an output beyond 2^60 floats.  count == 0 succeeds without a launch.  The checks need no GPU.
 * ---------------------------------------------------------------------- */
int fno_data_gather(int src_dtype, int stat_dtype, const void* src, size_t n_src, size_t snap_elems, size_t offset,
                    size_t row_stride, size_t col_stride, int rows, int cols, const long long* idx, size_t count,
                    const void* mean, const void* std_, double eps, float* out, size_t out_stride, void* stream);

/* ------------------------------------------------------------------------
 * Device-resident PINO training data (libs/pino_utils/datasets.py DevicePinoBatches): a batch (u, a_in) of a
 * MultipleReynoldsKFaDataset from tensors that stay on the device, one launch each.  idx (count) int64 on the device picks the
 * entries.  Both kernels move 32-bit words, never floats: NaN payloads, infinities, -0.0 and denormals arrive unchanged.
 *
 * fno_data_transpose_gather: src is a pool of n_src entries of (rows, cols) float32; for entry e, r < rows, c < cols
 *     out[e * out_stride + c * rows + r] = src[idx[e] * rows * cols + r * cols + c]
 * (the dataset: rows = T frames of a window, cols = S * S; every entry a (T, S*S) -> (S*S, T) transpose).  The source is read in
 * whole runs along c (16-byte loads where the address allows), the layout turns in LDS, the destination is written in whole
 * 16-byte vectors along r laid over the output's address, so `out` needs the alignment of a float only and rows may be odd; rows
 * is not bounded (frame chunks), rows == 1 is a gather-copy.
 * FNO_EINVAL: a null src / idx / out, rows or cols < 1, out_stride < rows * cols, a tensor not aligned to its element size;
 * FNO_EUNSUPPORTED: a pool beyond 2^62 bytes or an output beyond 2^60 floats.
 *
 * fno_pino_input: a0 is a pool of n_src planes (s1, s2) float32, gx (s1), gy (s2), gt (t) the axis vectors of the grid;
 *     out[e, x, y, k, :] = (gx[x], gy[y], gt[k], a0[idx[e], x, y])          channels-last (count, s1, s2, t, 4)
 * one 16-byte store per grid point, a0 read once per (x, y).  FNO_EINVAL: a null a0 / idx / gx / gy / gt / out, s1, s2 or t < 1,
 * a tensor not aligned to its element size, out not aligned to 16 bytes; FNO_EUNSUPPORTED: the same two size limits.
 *
 * Both: every index is compared unsigned against n_src before it becomes an address; an entry whose index is out of range reads
 * nothing and all its outputs are NaN.  One launch, no workspace, no atomics, 64-bit addressing, capturable.  count == 0
 * succeeds without a launch.  The checks need no GPU.
 * ---------------------------------------------------------------------- */
int fno_data_transpose_gather(const float* src, size_t n_src, int rows, int cols, const long long* idx, size_t count, float* out,
                              size_t out_stride, void* stream);
int fno_pino_input(const float* a0, size_t n_src, const long long* idx, size_t count, const float* gx, const float* gy,
                   const float* gt, int s1, int s2, int t, float* out, void* stream);

/* ------------------------------------------------------------------------
 * Lifting layer on its own:  y = W x + b,  x (B, Cin <= 4, PW) -> y (B, C, PW), C in {32, 64}, PW % 128 == 0
 * (neuralop/models/tfno.py:11-20; also the `fc0` + Re-conditioning front of the PINO observers,
 * libs/models/pino_models/pinobserver.py:205-207, once its two linear maps are composed).  backward gives the
 * parameter gradients only (x is data).
 * ---------------------------------------------------------------------- */
size_t fno_lifting_workspace_bytes(int channels);
int fno_lifting_forward(int batch, int cin, int channels, size_t plane, const float* x, const float* w, const float* bias,
                        float* y, void* stream);
int fno_lifting_backward(int batch, int cin, int channels, size_t plane, const float* x, const float* dy, float* dw,
                         float* dbias, void* ws, size_t ws_bytes, void* stream);
/* dx[b][k][p] = sum_c w[c][k] dy[b][c][p], channels ascending: the input gradient, for the shapes fno_lifting_forward takes */
int fno_lifting_backward_dx(int batch, int cin, int channels, size_t plane, const float* dy, const float* w, float* dx,
                            void* stream);

/* ------------------------------------------------------------------------
 * Channel-flow Navier-Stokes right-hand side on the staggered grid and the physics-informed loss built on it:
 * NSControlEnvMatlab.compute_rhs_py (libs/envs/control_env.py:429-530) and NSControlEnvMatlab.pde_loss (:627-633),
 * the `pde_loss_weight` branch of the observer training loop (run_pde_observers.py:226-231).
 * One field: U, W (Nx, Ny+1, Nz), V (Nx, Ny, Nz), z contiguous; all calls take `batch` stacked fields.
 *   fno_chanflow_pack_metrics: HOST helper.  From the wall-normal grid y[Ny] (faces), ym[Ny-1] (centres),
 *     yg[Ny+1] (ghost-extended centres, control_env.py:165) fills packed[3*(Ny+2)] with the reciprocal spacings the
 *     kernels index; the caller copies `packed` (doubles) to the device once and passes it as `metrics`.
 *   fno_chanflow_rhs: Fu, Fv, Fw = compute_rhs_py(U, V, W, dPdx); dtype 0 = fp32, 1 = fp64 (the reference's RK3 stepper
 *     runs it in fp64, the training loop on fp32 fields); dpdx = per-sample device array of that dtype or NULL for
 *     `dpdx_default`.
 *   fno_chanflow_pde_loss_forward: loss = sum_b ||Fu(U,Vgt,W)-Fu(U,V,W)|| + ||Fv..|| + ||Fw..|| (fp32, device scalar);
 *     leaves the difference fields and per-sample norms in `ws`.
 *   fno_chanflow_pde_loss_backward: dV = gloss * dloss/dV (gloss: device scalar, NULL = 1); Vgt is data.
 * ---------------------------------------------------------------------- */
typedef struct FnoChanflowGrid {
  int Nx, Ny, Nz;        /* Ny = number of y faces (rows of V); U and W carry Ny+1 rows */
  double dx, dz, nu;
} FnoChanflowGrid;
int fno_chanflow_pack_metrics(int Ny, const double* y, const double* ym, const double* yg, double* packed);
int fno_chanflow_rhs(const FnoChanflowGrid* grid, int batch, int dtype, const double* metrics, const void* U, const void* V,
                     const void* W, const void* dpdx, double dpdx_default, void* Fu, void* Fv, void* Fw, void* stream);
size_t fno_chanflow_pde_loss_workspace_bytes(const FnoChanflowGrid* grid, int batch);
int fno_chanflow_pde_loss_forward(const FnoChanflowGrid* grid, int batch, const double* metrics, const float* U,
                                  const float* Vgt, const float* V, const float* W, float* loss, void* ws, size_t ws_bytes,
                                  void* stream);
int fno_chanflow_pde_loss_backward(const FnoChanflowGrid* grid, int batch, const double* metrics, const float* U,
                                   const float* Vgt, const float* V, const float* W, const float* gloss, float* dV, void* ws,
                                   size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Channel-flow environment step in float64: NSControlEnvMatlab.time_advance_RK3_py (libs/envs/control_env.py:533-580),
 * compute_projection_step (:582-613), compute_pressure_py / get_boundary_pressures (:196-229, :423-427) and the scores
 * (:186-303).  State layout as above with `batch` independent environments; dtype must be 1 (fp64: the (0,0) Poisson
 * system has condition number ~7e6, fp32 cannot hold the project's 1e-5 line).  Nx, Nz in 2..128, Ny >= 3.
 *   fno_chanflow_poisson_table_bytes / _pack: HOST helper.  Twiddles, the trapezoid weights of the bulk velocity and, for every
 *     wavenumber pair (kx, kz <= Nz/2), the Thomas factors of DD + (kxx[kx] + kzz[kz]) I (the (0,0) system with D[0,0] * 1.5):
 *     reciprocal pivots and forward multipliers.  The caller copies the table to the device once (16-byte aligned) and passes
 *     it with its size; a table of another grid is refused.
 *   fno_chanflow_project: U, V, W <- compute_projection_step(U, V, W), then the U, W ghost rows by reflection; in place.
 *   fno_chanflow_wall_pressure: p1, p2 (batch, Nx, Nz) = get_boundary_pressures(); P (batch, Nx, Ny-1, Nz) too unless NULL.
 *   fno_chanflow_rk3_step: one step_rk3(opV1, opV2) in place; opV1, opV2 (batch, Nx, Nz); dpdx (batch) in/out; meanU0 (batch).
 *   fno_chanflow_diagnostics: out (batch, 12) = sum(div), mean|U|, mean|V|, mean|W|, ||U||, ||V||, ||W||, |wall shear stress|,
 *     bulk velocity, mean(p2), finite-difference dPdx of p2, signed wall shear stress; p2 may be NULL (entries 9, 10 = 0).
 * All device work goes to `stream`: no allocation, no synchronisation, so a step can be captured into a graph.
 * ---------------------------------------------------------------------- */
#define FNO_CHANFLOW_DIAG_COUNT 12
size_t fno_chanflow_poisson_table_bytes(const FnoChanflowGrid* grid);
int fno_chanflow_poisson_pack(const FnoChanflowGrid* grid, const double* y, const double* ym, const double* yg, double* packed,
                              size_t packed_bytes);
size_t fno_chanflow_step_workspace_bytes(const FnoChanflowGrid* grid, int batch);
int fno_chanflow_project(const FnoChanflowGrid* grid, int batch, int dtype, const double* metrics, const double* table,
                         size_t table_bytes, void* U, void* V, void* W, void* ws, size_t ws_bytes, void* stream);
int fno_chanflow_wall_pressure(const FnoChanflowGrid* grid, int batch, int dtype, const double* metrics, const double* table,
                               size_t table_bytes, const void* U, const void* V, const void* W, const void* dpdx, void* p1,
                               void* p2, void* P, void* ws, size_t ws_bytes, void* stream);
int fno_chanflow_rk3_step(const FnoChanflowGrid* grid, int batch, int dtype, const double* metrics, const double* table,
                          size_t table_bytes, void* U, void* V, void* W, const void* opV1, const void* opV2, void* dpdx,
                          const void* meanU0, double dt, void* ws, size_t ws_bytes, void* stream);
int fno_chanflow_diagnostics(const FnoChanflowGrid* grid, int batch, int dtype, const double* metrics, const double* table,
                             size_t table_bytes, const void* U, const void* V, const void* W, const void* p2, void* out,
                             void* stream);

/* ----------------------------------------------------------------------
 * Closed-loop control (run_control.py): everything between the fp64 channel-flow state and the fp32 observers stays on the device.
 *   fno_ctrl_encode: x[b * x_batch_stride + i] = (float)((p[b][i] - mean[i]) / (std[i] + eps)), i < plane: fp64 arithmetic with
 *     a true division, one rounding to fp32 (NormalizerGivenMeanStd.encode, then .float()).  The stride lets the call write
 *     channel 0 of an NCHW (batch, 3, Nx, Nz) observer input (stride 3 * plane) or an RNO input (stride plane).
 *   fno_ctrl_decode: opV2[b][i] = (double)y[b * y_batch_stride + i] * (std[i] + eps) + mean[i] (product and sum rounded
 *     separately), then * scale, clamp to +-clip (0 = off), minus the sample's own plane mean (zero_mean != 0), in this order;
 *     the mean is a fixed-order sum inside one workgroup.  opV1 (may be NULL) is zero-filled.
 *   fno_chanflow_diagnostics2: the twelve entries of fno_chanflow_diagnostics and dpdx[b] as the thirteenth, written to
 *     out + b * out_stride (doubles; out_stride >= 13): one row of a (T, batch, 13) log.  Two launches: a workgroup per
 *     (wall-normal row, sample) leaves partial sums in `ws` (fno_chanflow_diagnostics2_workspace_bytes, exactly), a workgroup per
 *     sample adds them in a fixed order.  Run-to-run and batch-position invariant.
 *   fno_ctrl_stats_update: Welford update of per-point mean and M2 (double) with one more snapshot x of each field;
 *     `count` = number of snapshots including this one (count == 1 initialises mean and M2 without reading them).
 *     std = sqrt(M2 / count), the population form.  The table is passed by value to the kernel.
 * No allocation, no synchronisation: every call can be captured into a graph.
 * ---------------------------------------------------------------------- */
#define FNO_CTRL_STATS_MAX 8
typedef struct FnoCtrlStats {
  const double* x[FNO_CTRL_STATS_MAX];
  double* mean[FNO_CTRL_STATS_MAX];
  double* m2[FNO_CTRL_STATS_MAX];
  size_t n[FNO_CTRL_STATS_MAX];      /* points per field */
} FnoCtrlStats;
int fno_ctrl_encode(int batch, size_t plane, const double* p, const double* mean, const double* std_, double eps, float* x,
                    size_t x_batch_stride, void* stream);
int fno_ctrl_decode(int batch, size_t plane, const float* y, size_t y_batch_stride, const double* mean, const double* std_,
                    double eps, double scale, double clip, int zero_mean, double* opV1, double* opV2, void* stream);
size_t fno_chanflow_diagnostics2_workspace_bytes(const FnoChanflowGrid* grid, int batch);
int fno_chanflow_diagnostics2(const FnoChanflowGrid* grid, int batch, int dtype, const double* metrics, const double* table,
                              size_t table_bytes, const void* U, const void* V, const void* W, const void* p2, const void* dpdx,
                              void* out, size_t out_stride, void* ws, size_t ws_bytes, void* stream);
int fno_ctrl_stats_update(const FnoCtrlStats* table, int nfields, long long count, void* stream);

/* ----------------------------------------------------------------------
 * optimal-observer policy (run_control.py:186-224): Adam on the upper-wall action through the full-field observer.  Per
 * environment b, S = std + eps (float64 wall-plane statistics), a (batch, plane) the float32 action, P predicted planes:
 *   fno_ctrl_action_begin: a = (float)opV2_0; x[b * x_batch_stride + i] = (float)(((double)a - mean[i]) / S[i]): the leaf and the
 *     first observer input, one rounding each.
 *   fno_ctrl_action_objective: field = (double)y * S + mean over y (batch, P, plane); nf = sqrt(sum field^2), na = sqrt(sum a^2);
 *     parts[b] = {nf + reg * na, nf, na}; dy = (float)(field / nf * S) (0 where nf == 0).  Two launches, two passes over y: a
 *     workgroup per 1024 points leaves two partial sums in `ws` (fno_ctrl_action_workspace_bytes, exactly; 0 for a bad shape),
 *     then every workgroup adds its environment's partials in one fixed order.  Run-to-run and batch-position invariant.
 *   fno_ctrl_action_update: g = (float)((double)dx / S + reg * (double)a / na) (second term 0 where na == 0; na = parts[b][2]),
 *     one Adam step on (a, g) in fp32 with fno_adam_step's arithmetic (no weight decay; bias corrections of `step` formed on the
 *     host in double, fno_adam_scalars), and x = (float)(((double)a - mean) / S) for the next epoch, in one pass.  step == 1
 *     initialises exp_avg / exp_avg_sq without reading them.
 *   fno_ctrl_action_finish: opV2[b][i] = (double)a[b][i] - mean over the plane of (double)a[b]; the mean is a fixed-order sum
 *     inside one workgroup.
 * No allocation, no synchronisation, no atomics: every call can be captured into a graph.
 * ---------------------------------------------------------------------- */
size_t fno_ctrl_action_workspace_bytes(int batch, int planes, size_t plane);
int fno_ctrl_action_begin(int batch, size_t plane, const double* opV2_0, const double* mean, const double* std_, double eps,
                          float* a, float* x, size_t x_batch_stride, void* stream);
int fno_ctrl_action_objective(int batch, int planes, size_t plane, const float* y, const float* a, const double* mean,
                              const double* std_, double eps, double reg, double* parts, float* dy, void* ws, size_t ws_bytes,
                              void* stream);
int fno_ctrl_action_update(int batch, size_t plane, const float* dx, const double* parts, const double* mean, const double* std_,
                           double eps, double reg, double lr, double beta1, double beta2, double adam_eps, int step, float* a,
                           float* exp_avg, float* exp_avg_sq, float* x, size_t x_batch_stride, void* stream);
int fno_ctrl_action_finish(int batch, size_t plane, const float* a, double* opV2, void* stream);

/* ----------------------------------------------------------------------
 * optimal-policy-observer policy (run_control.py:162-185): a policy network maps the raw wall pressure to a correction `res`
 * of the opposition-control action and is trained on line through the frozen full-field observer.  The glue between the two
 * networks; every tensor is dense (batch, plane):
 *   fno_ctrl_policy_begin: a0 = (float)opV2_0 and pin = (float)p2, one launch: the start action and the policy's input (the
 *     RAW wall pressure, no normaliser).
 *   fno_ctrl_policy_compose: x = a0 + res (one fp32 add) and opV2 = (double)x in the same pass: the observer's input and the
 *     action the loop applies; what the last epoch leaves is the applied action, there is no finish kernel.
 *   fno_ctrl_policy_grad: g = (float)((double)dx + reg * (double)x / na), na = parts[b][2] of fno_ctrl_action_objective
 *     (g = dx where na == 0): dL/dres, assembled in fp64 and rounded once.
 * The objective between compose and grad is fno_ctrl_action_objective with a := x and unit statistics (mean 0, std 1, eps 0).
 * No allocation, no synchronisation, no atomics: every call can be captured into a graph.
 * ---------------------------------------------------------------------- */
int fno_ctrl_policy_begin(int batch, size_t plane, const double* opV2_0, const double* p2, float* a0, float* pin, void* stream);
int fno_ctrl_policy_compose(int batch, size_t plane, const float* a0, const float* res, float* x, double* opV2, void* stream);
int fno_ctrl_policy_grad(int batch, size_t plane, const float* dx, const float* x, const double* parts, double reg, float* g,
                         void* stream);

/* ----------------------------------------------------------------------
 * NSControlEnv2D (libs/envs/ns_control_2d.py): the 2-D periodic channel with wall blowing and suction, float64.  Arrays are
 * (batch, ny, nx), row = wall-normal index, column = streamwise index, periodic in x with all nx columns distinct; `batch`
 * independent environments, one workgroup each, the whole state in LDS for the whole launch.  3 <= ny, nx and
 * ny * nx <= FNO_NS2D_MAX_POINTS (seven float64 planes in 160 KB of LDS); anything beyond returns FNO_EUNSUPPORTED.
 *   fno_ns2d_solve: NSControlEnv2D.solve (:359-491) from (p, u, v) with per-environment F[batch], nu[batch] and wall velocities
 *     bc_lo, bc_hi (batch, nx) (NULL: zero): steps while udiff > u_diff_thre; more than step_cap steps end the launch with
 *     status 2 (the reference's "Not converged solving!", step_cap = 5000 there) and max_step > 1 caps with status 1; status 0
 *     = converged.  out (batch, 3) = bulk_v (mean|u|), steps, status.  update_state != 0 writes p, u, v in place (and un, vn
 *     unless NULL) unless the cap was hit.
 *   fno_ns2d_fixed_mass: solve_fixed_mass (:493-536): converged solves at min_f[b] and max_f[b], then bisection on F towards
 *     target[b] while error > error_threshold, at most max_bisect times, all in one launch.  out (batch, 6) = result_f, flow,
 *     error, bisections, total steps, status (0 ok, 1 target outside the bracket: (F[b], target, 0) as the reference returns,
 *     2 a solve hit step_cap).  The state is read only.
 *   fno_ns2d_diagnostics: out (batch, 7) = the drag_reduction scalars of step (:562-581) in the order of `info`: |wall shear
 *     stress|, mean|u|, mean|v|, mean(p[-1,:]), dpdx[b] (NULL: -1), -|divergence| at the fixed indices 10 and 9 (so ny, nx >= 11),
 *     ||v|| + ||u||; ptop (batch, nx) = p[-1, :].
 * Every sum is a fixed-order reduction inside one workgroup: run-to-run, batch-size and batch-position invariant.  No
 * allocation, no synchronisation.
 * ---------------------------------------------------------------------- */
#define FNO_NS2D_MAX_POINTS 2907
#define FNO_NS2D_SOLVE_OUT 3
#define FNO_NS2D_FIXED_OUT 6
#define FNO_NS2D_DIAG_OUT 7
typedef struct FnoNs2dGrid {
  int nx, ny, nit;
  double dx, dy, dt, rho;
} FnoNs2dGrid;
int fno_ns2d_solve(const FnoNs2dGrid* grid, int batch, void* p, void* u, void* v, void* un, void* vn, const void* F,
                   const void* nu, const void* bc_lo, const void* bc_hi, int max_step, double u_diff_thre, int step_cap,
                   int update_state, void* out, void* stream);
int fno_ns2d_fixed_mass(const FnoNs2dGrid* grid, int batch, const void* p, const void* u, const void* v, const void* F,
                        const void* nu, const void* target, const void* min_f, const void* max_f, const void* bc_lo,
                        const void* bc_hi, double u_diff_thre, int step_cap, int max_bisect, double error_threshold, void* out,
                        void* stream);
int fno_ns2d_diagnostics(const FnoNs2dGrid* grid, int batch, const void* p, const void* u, const void* v, const void* nu,
                         const void* dpdx, void* out, void* ptop, void* stream);

/* Names and average device time (ms, HIP events on `stream`) of the kernels launched
 * by the last fno_model_* call made with profiling enabled; used by bench.py for the
 * roofline line.  fno_profile_enable(1) makes every launch event-bracketed (slow path). */
void fno_profile_enable(int on);
int fno_profile_count(void);
int fno_profile_get(int idx, const char** name, float* total_ms, int* launches);
/* which matrix pipe record idx's channel GEMMs ran on: 0 not stated, 1 fp32 MFMA, 2 two fp16 terms per operand (3 products per
 * k block), 3 three bf16 terms (6 products) - what a roofline has to price the kernel against */
int fno_profile_get_terms(int idx);
void fno_profile_reset(void);

#ifdef __cplusplus
}
#endif
#endif
