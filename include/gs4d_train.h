/*
 * gs4d_train.h -- C ABI of libgs4d's train-step kernels: the rows SURVEY.md §8f lists on either side
 * of the rasterizer (the HexPlane deformation field before it, the loss / densification statistics /
 * optimizer after it).  Each entry point replaces a PyTorch formulation of the reference; the
 * reference file:line it restates is given with it.  Same conventions as gs4d.h: device pointers,
 * fp32, C-contiguous, launches enqueued on `stream`, status 0 = OK, 1 = bad argument, 3 = HIP error.
 */
#ifndef GS4D_TRAIN_H_INCLUDED
#define GS4D_TRAIN_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#include "gs4d.h" /* gs4d_alloc_fn and the status codes (gs4d_isometry_loss_grad) */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- L1 loss: utils/loss_utils.py:20-21 l1_loss(x, y) = |x - y|.mean(), and its autograd gradient.
 * forward: *loss = mean |x - y| (fp64 partial sums in a fixed order), sign[i] = sign(x[i] - y[i]);
 * scratch must hold gs4d_l1_scratch_bytes(n) bytes and be all zero on entry (the completion counters and
 * partial slots of the workgroup that finishes last: it sums the partials itself, no second launch); a call
 * leaves it zero again, so a caller zeroes its scratch once and keeps it (one scratch per stream: two calls
 * in flight at once must not share one).  backward: grad[i] = sign[i] * (*dloss) / n. */
size_t gs4d_l1_scratch_bytes(int64_t n);
int gs4d_l1_loss_forward(int64_t n, const float *x, const float *y, int8_t *sign, float *loss, void *scratch,
                         void *stream);
/* Value AND gradient in one pass, for an upstream gradient `dloss` known on the host (a training step's
 * loss.backward() with dloss = 1): grad = sign(x - y) * (dloss * (1 / n)), bitwise what
 * gs4d_l1_loss_forward + gs4d_l1_loss_backward give, without writing and re-reading the signs.  n % 4 == 0 and
 * 16-byte aligned x, y, grad (GS4D_ERR_ARG otherwise). */
int gs4d_l1_loss_grad(int64_t n, const float *x, const float *y, float dloss, float *loss, float *grad, void *scratch,
                      void *stream);
int gs4d_l1_loss_backward(int64_t n, const int8_t *sign, const float *dloss, float *grad, void *stream);

/* ---- depth + mask supervision of one view (this build's opt-in; no reference counterpart: the reference's
 * Camera carries `depth` and `mask`, scene/cameras.py:21,54, and no loss reads them).  Over the n pixels of the
 * depth image and the alpha image (gs4d_alpha_image), with valid = gt_depth > 0 and n_valid = max(1, count(valid))
 * counted on the device (no host readback):
 *   *loss        = w_depth * (sum over valid of |depth - gt_depth|) / n_valid + w_mask * (sum |alpha - gt_mask|) / n
 *   dL_ddepth[i] = w_depth * sign(depth[i] - gt_depth[i]) / n_valid where valid, 0 elsewhere
 *   dL_dalpha[i] = w_mask * sign(alpha[i] - gt_mask[i]) / n                          (sign(0) = 0)
 * A NULL gt_depth or gt_mask drops that term; its inputs are then not read, its gradient image is not written
 * and both may be NULL.  Any n >= 1.  Two launches; the sums run in a fixed order (fp64 partials per 2048
 * pixels, totalled alike by every workgroup), so the value and both images are bitwise repeatable.  scratch:
 * gs4d_aux_loss_scratch_bytes(n) bytes, contents irrelevant on entry (one scratch per stream).
 * Status: 1 for n < 1, a NULL loss or scratch, or a NULL image of a term that is present. */
size_t gs4d_aux_loss_scratch_bytes(int64_t n);
int gs4d_aux_loss_grad(int64_t n, const float *depth, const float *alpha, const float *gt_depth, const float *gt_mask,
                       float w_depth, float w_mask, float *loss, float *dL_ddepth, float *dL_dalpha, void *scratch,
                       void *stream);

/* ---- SSIM / D-SSIM: utils/loss_utils.py:36-66 ssim(img1, img2, window_size=11, size_average): the 11x11
 * Gaussian window (sigma 1.5, normalised), zero padding of 5, one filter per channel, C1 = 0.01^2,
 * C2 = 0.03^2, map = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)), applied separably
 * (11 taps along the rows, then 11 along the columns) in one launch per direction.  x, y (B, C, H, W).
 * Status 1 for a null pointer or a negative dimension; a zero dimension is an empty batch: status 0, no
 * launch, the values zeroed.  H * W < 2^31, B <= 65535.
 * scratch: gs4d_ssim_scratch_bytes(B, C, H, W) bytes, all zero on entry and left zero, kept by the caller as
 * the L1 loss's above (the totals are fp64 partials per 32x32 tile summed in a fixed order per image, then
 * over the images in order: bitwise repeatable). */
size_t gs4d_ssim_scratch_bytes(int B, int C, int H, int W);
/* *mean = map.mean() (size_average=True), per_image[b] = map[b].mean() (size_average=False).  maps: NULL for
 * the values only, else 3 * B*C*H*W floats that receive what gs4d_ssim_backward needs (the map's derivatives
 * by the three filtered moments of x that it depends on). */
int gs4d_ssim_forward(int B, int C, int H, int W, const float *x, const float *y, float *maps, float *mean,
                      float *per_image, void *scratch, void *stream);
/* grad_x = the gradient autograd derives for img1: dvalue (device) is the upstream gradient of the mean
 * (per_image = 0: one float) or of the B per-image means (per_image = 1: B floats); each is divided by the
 * element count it averages over.  A gather: no atomics, each element written once.  y gets no gradient. */
int gs4d_ssim_backward(int B, int C, int H, int W, const float *x, const float *y, const float *maps,
                       const float *dvalue, int per_image, float *grad_x, void *stream);
/* The train step's image loss, train.py:244 + :255-257, value and gradient in two launches for an upstream
 * gradient known on the host (as gs4d_l1_loss_grad): *l1 = mean |x - y|, *ssim = ssim(x, y) (the mean over
 * everything), grad_x = d/dx of dloss * (l1 + lambda * (1 - ssim)).  maps: 3 * B*C*H*W floats of workspace
 * (caller-provided); scratch as gs4d_ssim_forward's. */
int gs4d_l1_dssim_loss_grad(int B, int C, int H, int W, const float *x, const float *y, float lambda, float dloss,
                            float *maps, float *l1, float *ssim, float *grad_x, void *scratch, void *stream);

/* ---- the deformation's tail and the activations before the rasterizer, in one pass each way:
 * scene/deformation.py:140-146 (residual adds of the heads' outputs, features = cat(f_dc, f_rest),
 * scene/gaussian_model.py:116-118) and gaussian_renderer/__init__.py:97-99 (exp, normalize, sigmoid):
 *   means = xyz + dx, scales = exp(s + ds), rot = (r + dr) / max(|r + dr|, 1e-12), opac = sigmoid(o + do),
 *   shs[:, 0] = f_dc + dshs[:, 0:3], shs[:, 1:] = f_rest + dshs[:, 3:] (K = 1 + K_rest coefficients).
 * Any delta may be NULL (that head is off: zero).  xyz, s (P, 3), r (P, 4), o (P, 1), f_dc (P, 1, 3),
 * f_rest (P, K-1, 3), dshs (P, 3K).  backward: given the gradients of the five outputs (each may be
 * NULL: zero), writes d xyz, d s, d r, d o, d f_dc and d f_rest (the slices of d shs, whose flat
 * (P, 3K) form is also the gradient of dshs), and the same values again into the deltas' gradients
 * g_dx, g_ds, g_dr, g_do where those are not NULL (separate buffers: autograd hands them to other
 * functions while the bases' gradients may become leaf .grad tensors).  d r is F.normalize's gradient,
 * g / max(n, eps) - [n > eps] q (q . g) / n^3 with q = r + dr, n = |q|, eps = 1e-12: g / eps at or below eps, finite
 * for a zero quaternion. */
int gs4d_deform_tail_forward(int P, int K, const float *xyz, const float *s, const float *r, const float *o,
                             const float *f_dc, const float *f_rest, const float *dx, const float *ds, const float *dr,
                             const float *d_o, const float *dshs, float *means, float *scales, float *rot,
                             float *opac, float *shs, void *stream);
int gs4d_deform_tail_backward(int P, int K, const float *scales, const float *r, const float *dr, const float *opac,
                              const float *g_means, const float *g_scales, const float *g_rot, const float *g_opac,
                              const float *g_shs, float *d_xyz, float *d_s, float *d_r, float *d_o, float *d_fdc,
                              float *d_frest, float *g_dx, float *g_ds, float *g_dr, float *g_do, void *stream);

/* ---- split-K partial sums: out[i] = sum over s = 0 .. S-1 of parts[s * n + i], in a fixed order that depends
 * only on S, n and the pointers' alignment (the same bits on every run):
 *   - S < 16, or n % 4 != 0, or parts / out not 16-byte aligned, or n > 2^26: slice order, s = 0, 1, .., S-1;
 *   - else four quarters, quarter q = the slices [q S / 4, (q + 1) S / 4) (integer division) added in slice
 *     order onto +0.0f, then out[i] = (q0 + q1) + (q2 + q3).
 * The deformation MLP's weight gradients dW = dY^T X over P ~ 1e5 rows are split-K GEMMs
 * (gs4d_train/deformation.py _splitk_dw) whose per-chunk results this adds in one pass. */
int gs4d_sum_slices(const float *parts, int S, int64_t n, float *out, void *stream);

/* ---- densification statistics: train.py:346-349 and scene/gaussian_model.py:521-523.
 * For every i with visible[i]: max_radii[i] = max(max_radii[i], radii[i]) (skipped when radii is
 * NULL), grad_accum[i] += |viewspace_grad[i, 0:2]|, denom[i] += 1.  viewspace_grad is (P, 3).  visible may
 * be NULL when radii is given: the mask is then radii[i] > 0, train.py:229-232's own definition of it. */
int gs4d_densify_stats(int P, const float *viewspace_grad, const uint8_t *visible, const int *radii, float *grad_accum,
                       float *denom, float *max_radii, void *stream);

/* ---- Adam: torch.optim.Adam(params, lr, betas=(0.9, 0.999), eps=1e-15) as built by
 * scene/gaussian_model.py:165-184, one launch for up to GS4D_ADAM_MAX_TENSORS tensors.  Per element:
 *   m = m + (1 - beta1) (g - m);  v = beta2 v + (1 - beta2) g^2;
 *   p = p + neg_step_size * m / (sqrt(v) / bias_correction2_sqrt + eps)
 * with neg_step_size = -lr / (1 - beta1^step) and bias_correction2_sqrt = sqrt(1 - beta2^step)
 * computed by the caller in double precision (as torch does).  first_chunk of tensor i must be the
 * sum of gs4d_adam_chunks(n) over tensors 0..i-1. */
#define GS4D_ADAM_MAX_TENSORS 48
typedef struct {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    int64_t n;
    int64_t first_chunk;
    float neg_step_size;
    float bias_correction2_sqrt;
} gs4d_adam_tensor;
typedef struct {
    int count;
    float beta1, one_minus_beta1, beta2, one_minus_beta2, eps;
    gs4d_adam_tensor t[GS4D_ADAM_MAX_TENSORS];
} gs4d_adam_batch;
int64_t gs4d_adam_chunks(int64_t n);
int gs4d_adam_step(const gs4d_adam_batch *batch, void *stream);

/* ---- Row surgery of densification and pruning: scene/gaussian_model.py:316-506 (prune_points,
 * densification_postfix, densify_and_clone, densify_and_split, and the optimizer-state edits they make).
 * One call rebuilds every per-Gaussian tensor (parameters, their Adam moments, statistics, the deformation
 * table) by one ROW PLAN: output row r < K is old row keep[r]; the A appended rows K + j are, per tensor mode:
 * GATHER -- old row append[j] for j < A - given_rows, then given[j - (A - given_rows)] (rows the caller
 * computed, e.g. a split's children's positions); ZERO_NEW -- zero (the new rows' Adam moments).  ZERO makes
 * every output row zero (the statistics the reference resets after densifying; src unused).  A copy is a copy:
 * the result is bitwise the reference's cat / boolean-index sequence, in its row order.  Elements are 1 or 4
 * bytes; rows are `width` elements, contiguous. */
#define GS4D_ROWS_MAX_TENSORS 32
enum { GS4D_ROWS_GATHER = 0, GS4D_ROWS_ZERO_NEW = 1, GS4D_ROWS_ZERO = 2 };
typedef struct {
    const void *src;    /* (P, width) old rows */
    const void *given;  /* (given_rows, width): the last appended rows of a GATHER tensor */
    void *dst;          /* (K + A, width) */
    int64_t width;
    int64_t given_rows; /* 0 <= given_rows <= A */
    int esize;          /* 1 or 4 */
    int mode;
} gs4d_rows_tensor;
typedef struct {
    int count;
    int64_t K, A;
    const int32_t *keep;    /* K old row indices, in output order */
    const int32_t *append;  /* old row indices of the gathered appended rows (A - given_rows of them per tensor) */
    gs4d_rows_tensor t[GS4D_ROWS_MAX_TENSORS];
} gs4d_rows_batch;
int gs4d_rows_assemble(const gs4d_rows_batch *batch, void *stream);

/* ---- HexPlane field: scene/hexplane.py:75-110 interpolate_ms_features (concat_features=True) over the
 * planes of init_grid_param (:50-72), each sampled with F.grid_sample(align_corners=True, bilinear,
 * padding_mode="border") (:22-48).  pts: (N, 4) normalised (x, y, z, t), 16-byte aligned.
 * feat: (N, levels * F) = for each level the product over the 6 coordinate pairs (0,1) (0,2) (0,3)
 * (1,2) (1,3) (2,3) of the pair's bilinear sample.  Plane 6*l + p of level l is a (1, F, H, W)
 * parameter tensor with W = reso[c0], H = reso[c1]; the kernels read a packed channels-last copy
 * of all planes (gs4d_hexplane_pack); the backward writes the plane gradients (every element: no zero
 * fill needed) into a packed buffer that gs4d_hexplane_unpack writes back to (1, F, H, W) gradient
 * tensors.  dpts receives the gradient w.r.t. pts (all 4 columns).  The plane gradients are always bitwise
 * reproducible: every term is rounded once to a 64-bit fixed-point integer and the integer sums (LDS windows
 * per workgroup, integer atomics across workgroups) are exact; `deterministic` is accepted and ignored (the
 * round-4 ABI's float-atomic mode is gone).  scratch: gs4d_hexplane_backward_scratch_bytes, required.  When
 * every lay->plane[p].grad is set, the gradients are written straight to those (1, F, H, W) tensors and
 * dpacked may be NULL (no packed round trip, no unpack call); otherwise dpacked receives them. */
#define GS4D_HEXPLANE_MAX_LEVELS 4
typedef struct {
    int W, H;
    int64_t offset; /* first float of the plane in the packed buffer: (H, W, F) */
    const float *param; /* (1, F, H, W) parameter (pack source) */
    float *grad;        /* (1, F, H, W) gradient (unpack destination) */
} gs4d_hexplane_plane;
typedef struct {
    int levels, F; /* F: features per plane, a multiple of 4 with F / 4 a power of two */
    int64_t total; /* floats in the packed buffer */
    gs4d_hexplane_plane plane[6 * GS4D_HEXPLANE_MAX_LEVELS];
} gs4d_hexplane_layout;
/* Fills offsets/total from the per-plane sizes W[6*levels], H[6*levels] (each side 1..65535, at most 2^31 - 1 cells
 * per plane); param/grad pointers are set by the caller. */
int gs4d_hexplane_layout_init(gs4d_hexplane_layout *lay, int levels, int F, const int *W, const int *H);
int gs4d_hexplane_pack(const gs4d_hexplane_layout *lay, float *packed, void *stream);
int gs4d_hexplane_unpack(const gs4d_hexplane_layout *lay, const float *packed, void *stream);
/* Visiting order of the points (a 3-D Morton order of the normalised x, y, z; any permutation of 0..N-1
 * gives the same results up to float summation order, NULL = identity).  Morton-consecutive points touch
 * small boxes of cells, which the backward's per-workgroup tap sort and gather exploit. */
size_t gs4d_hexplane_order_scratch_bytes(int N);
int gs4d_hexplane_order(int N, const float *pts, uint32_t *order, void *scratch, void *stream);
int gs4d_hexplane_forward(int N, const float *pts, const uint32_t *order, const gs4d_hexplane_layout *lay,
                          const float *packed, float *feat, void *stream);
/* scratch of gs4d_hexplane_backward: the scale words and 64-bit accumulators for the packed buffer */
size_t gs4d_hexplane_backward_scratch_bytes(int N, const gs4d_hexplane_layout *lay);
int gs4d_hexplane_backward(int N, const float *pts, const uint32_t *order, const gs4d_hexplane_layout *lay,
                           const float *packed, const float *dfeat, float *dpacked, float *dpts, void *scratch,
                           int deterministic, void *stream);
/* How the backward serves F features (host only, launches nothing; taken from the functions the kernel uses):
 * *points_per_workgroup consecutive points of the order share a workgroup, and a plane whose touched box of nc
 * cells fits *window_words 64-bit words at fp features per pass (fp = F, F/2, ... 4: the first with nc * fp <=
 * window_words) is summed in an LDS window, a larger one by direct atomics.  Nonzero for an F that
 * gs4d_hexplane_layout_init refuses. */
int gs4d_hexplane_backward_plan(int F, int *points_per_workgroup, int *window_words);

/* ---- The field's input points, scene/hexplane.py:20-21 (normalize_aabb with aabb = (max corner, min corner))
 * + :166 (torch.cat((pts, timestamps), -1)) in one pass: pts (N, 4) = ((xyz - aabb[0]) * s - 1, t) with
 * s = (1 / (aabb[1] - aabb[0])) * 2, the reference's float operations; xyz rows ld_xyz floats apart, t rows
 * ld_t apart (ld_t 0: one time for every point), aabb (2, 3) on the device, pts 16-byte aligned.  backward: dxyz (N, 3) = dpts[:, :3] * s. */
int gs4d_hexplane_points(int N, const float *xyz, int64_t ld_xyz, const float *t, int64_t ld_t, const float *aabb,
                         float *pts, void *stream);
int gs4d_hexplane_points_backward(int N, const float *dpts, const float *aabb, float *dxyz, void *stream);
/* The same with add (nullable, (N, 3) contiguous): dxyz = add + the points' gradient -- xyz's other gradient
 * (the deformation tail's, xyz + dx) summed in by this pass instead of a separate add. */
int gs4d_hexplane_points_backward_add(int N, const float *dpts, const float *aabb, const float *add, float *dxyz,
                                      void *stream);

/* ---- HexPlane regularisers: scene/gaussian_model.py:538-577 (compute_regulation = plane_tv_weight *
 * _plane_regulation + time_smoothness_weight * _time_regulation + l1_time_planes * _l1_regulation) with
 * scene/regulation.py:22-28 compute_plane_smoothness.  For every plane t (1, C, H, W) of the batch:
 *   w_smooth * mean over (C, H-2, W) of ((t[y+2] - t[y+1]) - (t[y+1] - t[y]))^2  +  w_l1 * mean |1 - t|
 * (w_smooth: plane_tv_weight for the spatial planes, time_smoothness_weight for the time planes; w_l1:
 * l1_time_planes for the time planes, 0 otherwise).  H >= 3.  forward: *loss = the sum over the
 * batch (fp64 partials summed in a fixed order; scratch of gs4d_reg_scratch_bytes, all zero on entry and left
 * zero, as the L1 loss's above).  backward: grad
 * (1, C, H, W) of each plane = dloss * d(loss)/d(t), the gradient autograd derives from the
 * reference's graph: assigned, or with accumulate = 1 added to what grad holds (the plane's .grad after
 * the field's backward: the sum autograd would form, without its extra add per plane).  first_block of
 * plane i = the sum of gs4d_reg_blocks over planes 0..i-1. */
#define GS4D_REG_MAX_PLANES 24
typedef struct {
    const float *data;
    float *grad;
    int C, H, W;
    float w_smooth, w_l1;
    int64_t first_block;
} gs4d_reg_plane;
typedef struct {
    int count;
    int accumulate;
    gs4d_reg_plane p[GS4D_REG_MAX_PLANES];
} gs4d_reg_batch;
int64_t gs4d_reg_blocks(int C, int H, int W);
size_t gs4d_reg_scratch_bytes(const gs4d_reg_batch *batch);
int gs4d_hexplane_reg_forward(const gs4d_reg_batch *batch, float *loss, void *scratch, void *stream);
int gs4d_hexplane_reg_backward(const gs4d_reg_batch *batch, const float *dloss, void *stream);
/* The backward and the value in one pass over the planes: the gradient as gs4d_hexplane_reg_backward, and *loss
 * bitwise as gs4d_hexplane_reg_forward would give it (same partials, same order); scratch as for the forward.
 * base (nullable): *loss = *base + value instead (one fp32 add: the loss term the value joins). */
int gs4d_hexplane_reg_backward_value(const gs4d_reg_batch *batch, const float *dloss, float *loss, const float *base,
                                     void *scratch, void *stream);

/* ---- Linear-layer weight gradients over many rows: for each problem, dw (n, W) = dy^T x and db (n)
 * = column sums of dy (db may be NULL) -- the backward of F.linear as autograd forms it -- for dy (P, n)
 * and x (P, W) given with row strides ld_dy >= n and ld_x >= W (x may be a column block of a wider
 * matrix).  Up to 8 problems with the same P and W per call; n <= 16 or n = 48, n * W <= 8192,
 * W in {64, 128, 256}.  Replaces the weight/bias gradients of the deformation heads' second layers
 * (scene/deformation.py:73-78, 152-164).  fp32, partial sums reduced in a fixed order. */
typedef struct gs4d_dw_problem {
    const float *dy;
    const float *x;
    float *dw;
    float *db;
    int n, ld_dy, ld_x;
} gs4d_dw_problem;
size_t gs4d_linear_dw_scratch_bytes(int P, int W, int count, const int *n);
int gs4d_linear_dw(int P, int W, int count, const gs4d_dw_problem *problems, void *scratch, void *stream);

/* ---- The deformation heads' second layers, backward (scene/deformation.py:73-78, evaluated as one
 * block: a = relu(h W1^T + b1) of shape (P, kW), head i = a[:, iW:(i+1)W] W2_i^T + b2_i), in one pass
 * over a: da = (a > 0) * [g_0 W2_0 | ... | g_{k-1} W2_{k-1}] (P, kW), db1 = column sums of da, and for each
 * head dW2_i = g_i^T a_i (n_i, W), db2_i = column sums of g_i -- what autograd forms with k mm, one
 * threshold_backward, a sum and 2k weight/bias reductions.  W in {64, 128, 256}, k W <= 768, n_i <= 16
 * or n_i = 48 (then W <= 128); g_i (P, n_i) contiguous (16-byte aligned when n_i = 48), a and da (P, kW) contiguous,
 * W2_i (n_i, W).  fp32, partial sums
 * reduced in a fixed order. */
#define GS4D_HEADS_MAX 8
typedef struct gs4d_heads_bwd {
    int P, W, k;
    const float *a;
    float *da;
    float *db1;
    int n[GS4D_HEADS_MAX];
    const float *g[GS4D_HEADS_MAX];
    const float *w2[GS4D_HEADS_MAX];
    float *dw2[GS4D_HEADS_MAX];
    float *db2[GS4D_HEADS_MAX];
} gs4d_heads_bwd;
size_t gs4d_heads_backward_scratch_bytes(int P, int W, int k, const int *n);
int gs4d_heads_backward(const gs4d_heads_bwd *args, void *scratch, void *stream);
/* The same pass on the bf16 path: a and da bf16 (uint16 bits; da rounded once from the f32 products), the
 * sums and g, W2, dW2, db1, db2 fp32.  n_i <= 16, or n_i = 48 with W in {64, 128}.  Same scratch size. */
typedef struct gs4d_heads_bwd_bf16 {
    int P, W, k;
    const uint16_t *a;
    uint16_t *da;
    float *db1;
    int n[GS4D_HEADS_MAX];
    const float *g[GS4D_HEADS_MAX];
    const float *w2[GS4D_HEADS_MAX];
    float *dw2[GS4D_HEADS_MAX];
    float *db2[GS4D_HEADS_MAX];
} gs4d_heads_bwd_bf16;
int gs4d_heads_backward_bf16(const gs4d_heads_bwd_bf16 *args, void *scratch, void *stream);
/* The bf16 block's input gradient dh (P, W) fp32 = da (P, KW) bf16 @ W1 (KW, W), given W1^T (W, KW) bf16 (the block
 * forward's w1t); bf16 MFMA, fp32 accumulation.  KW a multiple of 64, W in {64, 128}, 16-byte aligned. */
int gs4d_mlp_dx_bf16(int P, int KW, int W, const uint16_t *da, const uint16_t *w1t, float *dh, void *stream);
/* Its weight gradient dW1 (KW, W) fp32 = da^T hb over the P rows (da (P, KW), hb (P, W) bf16; W = 128, KW a multiple
 * of W): per 1024-row chunk and head a bf16-MFMA block (LDS transpose reads), the ceil(P / 1024) chunks summed by
 * gs4d_sum_slices in its fixed order (above: a quarter tree from 16 chunks on). */
size_t gs4d_mlp_dw_bf16_scratch_bytes(int P, int KW, int W);
int gs4d_mlp_dw_bf16(int P, int KW, int W, const uint16_t *da, const uint16_t *hb, float *dw, void *scratch,
                     void *stream);
/* The fp32 block's input gradient dh (P, W) = da (P, KW) @ W1 (KW, W), given W1^T (W, KW) (the block forward's
 * w1t), f32 MFMA with f32 products and sums in one fixed order: the same bits in every process
 * (scene/deformation.py:73-78's heads, the input gradient autograd forms by one GEMM).  KW a multiple of 64, W in
 * {64, 128}; rows 16-byte aligned. */
int gs4d_mlp_dx_f32(int P, int KW, int W, const float *da, const float *w1t, float *dh, void *stream);
/* Its weight gradient dW1 (KW, W) = da^T h over the P rows (da (P, KW), h (P, W) row-major): per row chunk and
 * 64-row block of dW1 an f32-MFMA block, its waves summed in a fixed order, the chunks summed by gs4d_sum_slices in its fixed order
 * (above; scratch: gs4d_mlp_dw_f32_scratch_bytes).  The chunk count follows the device's compute-unit count (one
 * resident round of workgroups), so dW1's bits are the same on every run and process on one device model, but
 * may differ in the last places between devices with different CU counts. */
size_t gs4d_mlp_dw_f32_scratch_bytes(int P, int KW, int W);
int gs4d_mlp_dw_f32(int P, int KW, int W, const float *da, const float *h, float *dw, void *scratch, void *stream);

/* ---- The deformation field's first layer, backward, when feature_out is ONE Linear (defor_depth <= 1,
 * scene/deformation.py:51-55: hidden = x W^T + b) and every head begins with ReLU, so the heads read
 * h = relu(hidden).  Given g = dL/dh (P, Fout), h (P, Fout), x (P, Fin), W (Fout, Fin), one pass over the
 * rows (f32 MFMA, exact f32 products) writes what autograd forms with threshold_backward, two GEMMs and a
 * sum: dx = (g * (h > 0)) W (P, Fin), dW = (g * (h > 0))^T x (Fout, Fin), db = column sums of
 * g * (h > 0) (Fout); partial sums reduced in a fixed order.  (Fin, Fout) in {(32, 128), (48, 128), (64, 64),
 * (32, 64)}; contiguous; g, h, W 16-byte aligned; scratch of gs4d_feature_relu_backward_scratch_bytes.
 * (48, 128) is the HyperNeRF / DyCheck shape: multires [1, 2, 4] x output_coordinate_dim 16, net_width 128
 * (arguments/hypernerf/default.py:5-10, arguments/dycheck/default.py:5-10); (32, 128) DyNeRF / multipleview,
 * (64, 64) D-NeRF. */
int gs4d_feature_relu_forward(int P, int Fin, int Fout, const float *x, const float *w, const float *b, float *h,
                              void *stream);  /* h = relu(x W^T + b), f32 MFMA; same shapes; x, W 16-byte aligned */
/* The same, also writing h rounded to bf16 into hb (uint16 bits, (ceil(P/16)*16, Fout); its padding rows hold row
 * P - 1's values), the input gs4d_heads_block_forward_bf16 takes when its h is NULL.  hb NULL: as above. */
int gs4d_feature_relu_forward_hb(int P, int Fin, int Fout, const float *x, const float *w, const float *b, float *h,
                                 uint16_t *hb, void *stream);
size_t gs4d_feature_relu_backward_scratch_bytes(int P, int Fin, int Fout);
int gs4d_feature_relu_backward(int P, int Fin, int Fout, const float *g, const float *h, const float *x,
                               const float *w, float *dx, float *dw, float *db, void *scratch, void *stream);

/* ---- The deformation heads' second layers, forward (scene/deformation.py:73-78 as one block): given
 * a = relu(h W1^T + b1) (P, kW), out_i = a[:, iW:(i+1)W] W2_i^T + b2_i (P, n_i) for every head in one pass
 * over a (f32 MFMA, exact f32 products), where torch runs k GEMMs on column slices.  W in {64, 128, 256},
 * 1 <= k <= 8, 1 <= n_i <= 64, the W2s (n_i, W) 16-byte aligned and at most 64 KiB together; a contiguous,
 * 16-byte aligned; out_i (P, n_i) contiguous. */
typedef struct gs4d_heads_fwd {
    int P, W, k;
    const float *a;
    int n[GS4D_HEADS_MAX];
    const float *w2[GS4D_HEADS_MAX];
    const float *b2[GS4D_HEADS_MAX];
    float *out[GS4D_HEADS_MAX];
} gs4d_heads_fwd;
int gs4d_heads_forward(const gs4d_heads_fwd *args, void *stream);

/* ---- The whole heads block, forward: a = relu(h W1^T + b1) (P, kW) AND out_i = a[:, iW:(i+1)W] W2_i^T + b2_i
 * (P, n_i) in one pass (f32 MFMA, exact f32 products); a is written for the backward and not read back.
 * Replaces the (P x W) @ (W x kW) first-layer GEMM plus gs4d_heads_forward.  W in {64, 128}, 1 <= k <= 8,
 * 1 <= n_i <= 64; h (P, W), W1 (kW, W) = the heads' first-layer weights stacked, b1 (kW), a (P, kW) contiguous
 * and 16-byte aligned WITH ROOM FOR ceil(P / 16) * 16 ROWS (the padding rows receive don't-care values: the
 * kernel stores whole 16-row blocks unconditionally), W2_i (n_i, W) 16-byte aligned, out_i (P, n_i) contiguous. */
typedef struct gs4d_heads_block_fwd {
    int P, W, k;
    const float *h;
    const float *w1;
    const float *b1;
    float *a;
    float *w1t;  /* nullable: W1^T (W, kW), written for the backward's input gradient (gs4d_mlp_dx_f32) */
    int n[GS4D_HEADS_MAX];
    const float *w2[GS4D_HEADS_MAX];
    const float *b2[GS4D_HEADS_MAX];
    float *out[GS4D_HEADS_MAX];
} gs4d_heads_block_fwd;
int gs4d_heads_block_forward(const gs4d_heads_block_fwd *args, void *stream);
/* The same block on bf16 operands (hyper.mlp_dtype = "bf16"): h, W1, W2 rounded to bf16, fp32 accumulation
 * (v_mfma_f32_16x16x32_bf16), a = relu(z + b1) stored as bf16 (uint16 bits, (ceil(P/16)*16, kW)), out_i fp32.
 * hb (nullable): h rounded to bf16, (ceil(P/16)*16, W), for the backward's weight-gradient GEMM; w1t (nullable):
 * W1^T rounded to bf16 (W, kW), for its input gradient (gs4d_mlp_dx_bf16).  h NULL: hb is an INPUT instead, h
 * already rounded to bf16 (gs4d_feature_relu_forward_hb): read as bf16, not converted per head, not written.
 * Returns 4 (GS4D_TRAIN_ERR_LDS) when the device cannot give the kernel its LDS (also for the fp32 form). */
#define GS4D_TRAIN_ERR_LDS 4
typedef struct gs4d_heads_block_fwd_bf16 {
    int P, W, k;
    const float *h;
    const float *w1;
    const float *b1;
    uint16_t *a;
    uint16_t *hb;
    uint16_t *w1t;
    int n[GS4D_HEADS_MAX];
    const float *w2[GS4D_HEADS_MAX];
    const float *b2[GS4D_HEADS_MAX];
    float *out[GS4D_HEADS_MAX];
} gs4d_heads_block_fwd_bf16;
int gs4d_heads_block_forward_bf16(const gs4d_heads_block_fwd_bf16 *args, void *stream);

/* ---- The deformation network at inference, one launch from the field features to the rasterizer's inputs
 * (scene/deformation.py:51-55,73-78,97-146 and gaussian_renderer/__init__.py:94-99): feature_out with
 * defor_depth <= 1, the heads, forward_dynamic's residual adds, and render()'s activations.
 *   h = relu(feat Wf^T + bf);  for each head i: a_i = relu(h W1_i^T + b1_i), d_i = a_i W2_i^T + b2_i (P, n_i);
 *   means = xyz + d_pos, scales = s + d_scales, rot = r + d_rot, opac = o + d_opacity,
 *   shs = cat(f_dc, f_rest) + d_shs.reshape(P, 16, 3)
 * and with activate != 0 the activations of gs4d_deform_tail_forward above, with its eps and its shs layout of K
 * coefficients: scales = exp(.), rot = . / max(|.|, 1e-12), opac = sigmoid(.).  A role without a head passes its
 * base through (activated when activate is set); all five outputs are always written in full.  Nothing else is
 * written: no h, no a, no deltas.  f32 MFMA, exact f32 products, each point's sums in one fixed order (the same
 * bits whatever the point's row).
 * (F, W) in {(32, 128), (48, 128), (64, 64), (32, 64)} ((48, 128): the HyperNeRF / DyCheck configurations,
 * arguments/hypernerf/default.py:5-10 and arguments/dycheck/default.py:5-10); 1 <= k <= 5 heads, each role at most
 * once, n_i = 3, 3, 4, 1, 48 for
 * role pos, scales, rot, opacity, shs; an shs head needs K = 16.  Anything else is status 1 with a
 * gs4d_last_error() text, before any HIP call; P = 0 is a successful no-op; with no head at all the caller uses
 * gs4d_deform_tail_forward.  feat (P, F), wf (W, F), bf (W), w1 (kW, W) = the heads' first-layer weights stacked
 * in head order, b1 (kW), w2[i] (n_i, W), b2[i] (n_i); bases and outputs as gs4d_deform_tail_forward's.  feat, wf,
 * w1, w2[i], rot and shs 16-byte aligned.  GS4D_TRAIN_ERR_LDS when the device cannot give the kernel its LDS
 * (4 ((W + npad) (W + 8) + W (F + 8) + 2 W + npad) bytes, npad = the widest head's n rounded up to 16: 117,440
 * at (32, 128) with shs, 125,632 at (48, 128)). */
enum { GS4D_ROLE_POS = 0, GS4D_ROLE_SCALES = 1, GS4D_ROLE_ROT = 2, GS4D_ROLE_OPACITY = 3, GS4D_ROLE_SHS = 4 };
typedef struct gs4d_deform_infer_args {
    int P, F, W, K; /* points, field features, hidden width, SH coefficients */
    int k;          /* active heads */
    int activate;
    const float *feat, *wf, *bf, *w1, *b1;
    int role[5], n[5];
    const float *w2[5];
    const float *b2[5];
    const float *xyz, *s, *r, *o, *f_dc, *f_rest;
    float *means, *scales, *rot, *opac, *shs;
} gs4d_deform_infer_args;
int gs4d_deform_infer(const gs4d_deform_infer_args *args, void *stream);

/* ---- local-isometry regulariser over a K-NN graph (no reference counterpart; opt-in; csrc/rigidity.hip).
 * The graph is gs4d_knn_graph's (gs4d.h): nbr_idx (P x K), in_start (P + 1), in_edge (P x K).  With
 * r(v) = sqrt(v.v + 1e-12), E = P min(K, P - 1) and Delta_e = r(xb_i - xb_j) - r(xa_i - xa_j), j = nbr_idx[e]:
 *   *value = scale / E * sum over the valid edges e = (i, k) of w_e Delta_e^2      (weights == NULL: w = 1)
 *   dL_dxb[i] = 2 scale / E * [ sum_k w_ik Delta_ik (xb_i - xb_j) / r_b - sum_{e = (m, k) in in(i)} w_e Delta_e (xb_m - xb_i) / r_b ]
 *   dL_dxa[i] = the same over xa and r_a with the opposite sign.
 * A node sums its out-edges in ascending k, then its in-edges in in_edge order; the value is summed per workgroup
 * in a fixed tree and the workgroups' partials in fp64 in index order by a second launch: no atomics, two calls
 * give the same bits.  Either gradient pointer may be NULL: that side is skipped, the other side's bits are
 * unchanged.  Nothing synchronises; the scratch must stay valid until `stream` has run the two launches.
 * Status: GS4D_OK at once for P == 0; GS4D_ERR_ARG (message beginning "isometry:") for K outside 1..16, P < 0,
 * P K >= 2^30, or with P > 0 a NULL graph, position or value pointer or a NULL allocator, all before the allocator
 * is asked; GS4D_ERR_ALLOC when it returns NULL. */
int gs4d_isometry_loss_grad(int P, int K, const int32_t *nbr_idx, const int32_t *in_start, const int32_t *in_edge,
                            const float *weights, const float *xa, const float *xb, float scale, float *value,
                            float *dL_dxa, float *dL_dxb, gs4d_alloc_fn scratch_alloc, void *scratch_ctx, void *stream);

/* ---- MCMC densification (no reference counterpart; opt-in; csrc/mcmc.hip; 3DGS-MCMC, Kheradmand et al. 2024).
 * Conventions of every entry below: nothing synchronises; a scratch block must stay valid until `stream` has run
 * the call's launches; GS4D_ERR_ARG (message beginning "mcmc:") for a bad argument, before any launch and before
 * the allocator is asked; GS4D_ERR_ALLOC when the allocator returns NULL; GS4D_OK at once for P == 0 (and n == 0,
 * n_blocks == 0): nothing is read or written then.
 *
 * The generator is Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85) with
 * key (seed & 0xffffffff, seed >> 32) and counter (j, purpose, iteration, 0): j the row or draw index, purpose
 * GS4D_MCMC_NOISE / _RELOCATE / _GROW.  gs4d_mcmc_random_bits writes the four words of blocks 0 .. n_blocks - 1
 * (out: 4 n_blocks words). */
enum { GS4D_MCMC_NOISE = 0, GS4D_MCMC_RELOCATE = 1, GS4D_MCMC_GROW = 2 };
int gs4d_mcmc_random_bits(int n_blocks, uint64_t seed, uint32_t iteration, uint32_t purpose, uint32_t *out, void *stream);
/* n draws with replacement in proportion to opacity, exact and order-free.  opacity (P): ACTIVATED opacities.
 * w_i = (uint64)(min(o_i, 1) 2^32) where o_i > min_opacity, else 0; S = the inclusive 64-bit prefix sums; draw d
 * takes u = w0 | w1 << 32 of block d, t = mulhi64(u, S[P-1]) and draws[d] = the first i with S[i] > t.  counts (P):
 * the draws per row (integer atomics).  n_drawn (nullable, one int): n, or 0 when S[P-1] == 0 (no live row): counts
 * is then all zero and draws is not written.  Status 1 for P < 0, n < 0, min_opacity < 0 or NaN, or with P, n > 0 a
 * NULL opacity, draws, counts or allocator.  Scratch: 8 (P + ceil(P / 256)) + 256 bytes. */
int gs4d_mcmc_sample(int P, const float *opacity, float min_opacity, int n, uint64_t seed, uint32_t iteration,
                     uint32_t purpose, int32_t *draws, int32_t *counts, int32_t *n_drawn, gs4d_alloc_fn scratch_alloc,
                     void *scratch_ctx, void *stream);
/* The sources' correction, in place on the RAW opacity (P) and scaling (P, 3) of the rows with counts[r] > 0 (the
 * others are not written): n = min(counts[r] + 1, 51), o = sigmoid(raw o), o' = -expm1(log1p(-o) / n),
 * D = sum_{i=1..n} sum_{k=0..i-1} C(i-1, k) (-1)^k o'^(k+1) / sqrt(k+1) in fp64, s' = exp(raw s) o / D, o' clamped
 * to [min_opacity, 1 - FLT_EPSILON]; stores log(o' / (1 - o')) and log(s').  min_opacity in (0, 1). */
int gs4d_mcmc_relocate(int P, const int32_t *counts, float min_opacity, float *opacity_raw, float *scaling_raw,
                       void *stream);
/* The per-step noise, one launch, xyz (P, 3) in place: x += R diag(s^2) R^T (z g step_scale) with R of the
 * normalised raw quaternion (w, x, y, z; norm clamped at 1e-12), s = exp(raw scale),
 * g = 1 / (1 + exp(-100 ((1 - sigmoid(raw opacity)) - 0.995))), and z = normals[r] when normals (P, 3) is given,
 * else of block r (purpose GS4D_MCMC_NOISE): u_k = ((w_k >> 8) + 0.5) 2^-24, r0 = sqrt(-2 ln u_0),
 * r1 = sqrt(-2 ln u_2), z = (r0 cos 2 pi u_1, r0 sin 2 pi u_1, r1 cos 2 pi u_3). */
int gs4d_mcmc_noise(int P, float *xyz, const float *scaling_raw, const float *rotation_raw, const float *opacity_raw,
                    float step_scale, uint64_t seed, uint32_t iteration, const float *normals, void *stream);
/* *value = w_opacity mean(sigmoid(raw o)) + w_scale mean(exp(raw s)) (means over P and 3 P elements), and its
 * gradient ADDED into grad_opacity (P) and grad_scaling (P, 3) (either may be NULL: skipped).  The value: a tree per
 * workgroup of 256 rows, the workgroups' fp64 partials added in index order by a second launch; no float atomics:
 * two calls give the same bits.  Scratch: 8 ceil(P / 256) + 256 bytes. */
int gs4d_mcmc_reg_grad(int P, const float *opacity_raw, const float *scaling_raw, float w_opacity, float w_scale,
                       float *value, float *grad_opacity, float *grad_scaling, gs4d_alloc_fn scratch_alloc,
                       void *scratch_ctx, void *stream);
/* Rows rows[0 .. n-1] of `count` float tensors (P, width) set to zero in one launch (the Adam moments of relocated
 * and grown rows).  Duplicates are fine; an index outside [0, P) is skipped.  Status 1 for a NULL batch, count
 * outside 0 .. GS4D_ROWS_MAX_TENSORS, negative P or n, or with work to do a NULL row list, a NULL tensor or a width
 * outside 1 .. 2^20. */
typedef struct {
    float *data;
    int64_t width;
} gs4d_zero_rows_tensor;
typedef struct {
    int count;
    int64_t P, n;
    const int32_t *rows;
    gs4d_zero_rows_tensor t[GS4D_ROWS_MAX_TENSORS];
} gs4d_zero_rows_batch;
int gs4d_mcmc_zero_rows(const gs4d_zero_rows_batch *batch, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GS4D_TRAIN_H_INCLUDED */
