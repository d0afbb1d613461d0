/*
 * gs4d.h -- C ABI of libgs4d, the MI355X (gfx950) differentiable Gaussian rasterizer.
 *
 * Drop-in boundary for the reference's native layer
 *   submodules/depth-diff-gaussian-rasterization/cuda_rasterizer/rasterizer.h:20-85
 *   (CudaRasterizer::Rasterizer::{markVisible, forward, backward})
 * which the reference's torch glue (rasterize_points.cu:36-219) binds through pybind (ext.cpp:15-18).
 * Signatures keep the reference's argument order and meaning; the differences are the ones a C ABI
 * needs: std::function allocators become (function pointer, context) pairs, the stream is explicit,
 * errors are returned as a status code instead of C++ exceptions/__trap, and outputs of the
 * reference's return value (num_rendered) come back through an out-pointer.
 *
 * Conventions (identical to the reference):
 *   - all float arrays are fp32, C-contiguous, device pointers (hipMalloc'd / torch HIP tensors);
 *   - "not provided" optional inputs are NULL (the reference passes empty tensors -> nullptr,
 *     rasterize_points.cu:95-106; branches at forward.cu:205,241 and backward.cu:390,394);
 *   - matrices are 4x4 column-major flat (viewmatrix = world_view_transform, projmatrix =
 *     full_proj_transform of scene/cameras.py:61-66);
 *   - color/depth outputs are planar CHW: out_color[ch*H*W + y*W + x] (forward.cu:376-377);
 *   - every launch is enqueued on `stream`; the forward performs exactly one device->host copy of
 *     num_rendered on that stream (rasterizer_impl.cu:282), nothing else synchronises.
 * Scratch buffers are requested through the allocator callbacks; their contents are opaque and only
 * meaningful to the matching gs4d_backward call (GeometryState/BinningState/ImageState analogue,
 * rasterizer_impl.h:31-67).  The internal layout is this library's own, not the reference's.
 */
#ifndef GS4D_H_INCLUDED
#define GS4D_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Status codes */
#define GS4D_OK 0
#define GS4D_ERR_ARG 1          /* invalid argument (shape, degree, NULL where required) */
#define GS4D_ERR_ALLOC 2        /* allocator callback returned NULL */
#define GS4D_ERR_HIP 3          /* a HIP runtime call or kernel launch failed */
#define GS4D_ERR_PREFILTERED 4  /* prefiltered=1 but a point fails the near-plane test (auxiliary.h:156-160) */

/* Scratch allocator: returns a device pointer to at least `nbytes` bytes (16-byte aligned) that stays
 * valid until the matching backward has run, or NULL on failure.  Replaces the reference's
 * std::function<char*(size_t)> resize functors (rasterize_points.cu:27-33). */
typedef char *(*gs4d_alloc_fn)(void *ctx, size_t nbytes);

/* Replaces CudaRasterizer::Rasterizer::markVisible (rasterizer.h:24-29, rasterizer_impl.cu:141-153).
 * present[i] = 1 iff point i passes the near-plane test (auxiliary.h:139-164). */
int gs4d_mark_visible(int P, const float *means3D, const float *viewmatrix, const float *projmatrix,
                      uint8_t *present, void *stream);

/* Replaces CudaRasterizer::Rasterizer::forward (rasterizer.h:31-57, rasterizer_impl.cu:198-339).
 * radii may be NULL (internal radii are then used).  *num_rendered receives the number of
 * (tile, Gaussian) instances L.  Limits (GS4D_ERR_ARG beyond them): P < 2^30, L < 2^30, fewer than
 * 2^30 16x16 tiles. */
int gs4d_forward(gs4d_alloc_fn geometry_alloc, void *geometry_ctx, gs4d_alloc_fn binning_alloc, void *binning_ctx,
                 gs4d_alloc_fn image_alloc, void *image_ctx, int P, int D, int M, const float *background, int width,
                 int height, const float *means3D, const float *shs, const float *colors_precomp,
                 const float *opacities, const float *scales, float scale_modifier, const float *rotations,
                 const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix, const float *cam_pos,
                 float tan_fovx, float tan_fovy, int prefiltered, float *out_color, float *out_depth, int *radii,
                 int debug, void *stream, int *num_rendered);

/* Replaces CudaRasterizer::Rasterizer::backward (rasterizer.h:59-85, rasterizer_impl.cu:343-437).
 * R = num_rendered of the matching forward; geom/binning/image are the buffers it allocated.
 * scratch_alloc provides the backward's own temporary (per-instance gradient terms).
 * Unlike the reference (which requires zero-filled gradient buffers, rasterize_points.cu:153-161),
 * every element of every gradient output is written, so the buffers may be uninitialised.
 * dL_dconic may be NULL (the reference allocates it but never returns it). */
int gs4d_backward(int P, int D, int M, int R, const float *background, int width, int height, const float *means3D,
                  const float *shs, const float *colors_precomp, const float *scales, float scale_modifier,
                  const float *rotations, const float *cov3D_precomp, const float *viewmatrix,
                  const float *projmatrix, const float *campos, float tan_fovx, float tan_fovy, const int *radii,
                  char *geom_buffer, char *binning_buffer, char *image_buffer, const float *dL_dpix,
                  float *dL_dmean2D, float *dL_dconic, float *dL_dopacity, float *dL_dcolor, float *dL_dmean3D,
                  float *dL_dcov3D, float *dL_dsh, float *dL_dscale, float *dL_drot, gs4d_alloc_fn scratch_alloc,
                  void *scratch_ctx, int debug, void *stream);

/* The same three entry points for a view matrix handed over transposed (view_transposed = 1: the 16
 * floats hold the transpose of the column-major matrix, i.e. a (1, 4)-strided 4x4 view such as the
 * reference callers' world_view_transform.cuda(), gaussian_renderer/__init__.py:45).  Reading it in
 * place saves the caller a copy per call; view_transposed = 0 is the plain entry point.  projmatrix
 * is always the column-major flat layout. */
int gs4d_mark_visible_ex(int P, const float *means3D, const float *viewmatrix, const float *projmatrix,
                         uint8_t *present, void *stream, int view_transposed);
int gs4d_forward_ex(gs4d_alloc_fn geometry_alloc, void *geometry_ctx, gs4d_alloc_fn binning_alloc, void *binning_ctx,
                    gs4d_alloc_fn image_alloc, void *image_ctx, int P, int D, int M, const float *background,
                    int width, int height, const float *means3D, const float *shs, const float *colors_precomp,
                    const float *opacities, const float *scales, float scale_modifier, const float *rotations,
                    const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix,
                    const float *cam_pos, float tan_fovx, float tan_fovy, int prefiltered, float *out_color,
                    float *out_depth, int *radii, int debug, void *stream, int *num_rendered, int view_transposed);
int gs4d_backward_ex(int P, int D, int M, int R, const float *background, int width, int height,
                     const float *means3D, const float *shs, const float *colors_precomp, const float *scales,
                     float scale_modifier, const float *rotations, const float *cov3D_precomp,
                     const float *viewmatrix, const float *projmatrix, const float *campos, float tan_fovx,
                     float tan_fovy, const int *radii, char *geom_buffer, char *binning_buffer, char *image_buffer,
                     const float *dL_dpix, float *dL_dmean2D, float *dL_dconic, float *dL_dopacity,
                     float *dL_dcolor, float *dL_dmean3D, float *dL_dcov3D, float *dL_dsh, float *dL_dscale,
                     float *dL_drot, gs4d_alloc_fn scratch_alloc, void *scratch_ctx, int debug, void *stream,
                     int view_transposed);

/* gs4d_backward_ex with a gradient for the depth image (no reference counterpart; opt-in).  The reference
 * blends a depth image D = sum depth_i alpha_i T_i next to the colour (forward.cu:250,359,377; no background
 * term) and drops its gradient: _RasterizeGaussians.backward ignores grad_depth
 * (diff_gaussian_rasterization/__init__.py:100-101).  Here dL_ddepth (H * W floats, the gradient of
 * out_depth) is back-propagated as a fourth blended channel whose per-splat "colour" is the view depth:
 * it reaches dL_dopacity, dL_dmean2D, dL_dconic (hence dL_dcov3D, dL_dscale, dL_drot) and dL_dmean3D through
 * the formulas of the colour channels, and dL_dmean3D also takes (sum over pixels of alpha T dL_ddepth) times
 * the view matrix's depth row.  dL_dcolor and dL_dsh receive nothing from it.  dL_ddepth = 0 gives
 * gs4d_backward_ex's results bit for bit, and the results are bitwise repeatable like its own.
 * Status: GS4D_ERR_ARG for P < 0 or R < 0; GS4D_OK at once for P == 0; GS4D_ERR_ARG when dL_ddepth or
 * dL_dpix is NULL; everything else as gs4d_backward_ex. */
int gs4d_backward_depth(int P, int D, int M, int R, const float *background, int width, int height,
                        const float *means3D, const float *shs, const float *colors_precomp, const float *scales,
                        float scale_modifier, const float *rotations, const float *cov3D_precomp,
                        const float *viewmatrix, const float *projmatrix, const float *campos, float tan_fovx,
                        float tan_fovy, const int *radii, char *geom_buffer, char *binning_buffer, char *image_buffer,
                        const float *dL_dpix, const float *dL_ddepth, float *dL_dmean2D, float *dL_dconic,
                        float *dL_dopacity, float *dL_dcolor, float *dL_dmean3D, float *dL_dcov3D, float *dL_dsh,
                        float *dL_dscale, float *dL_drot, gs4d_alloc_fn scratch_alloc, void *scratch_ctx, int debug,
                        void *stream, int view_transposed);

/* The alpha image of a forward (no reference counterpart; opt-in): out_alpha[pix] = 1 - final_T[pix] =
 * sum alpha_i T_i, the accumulated alpha of the pixel, read from the image state a gs4d_forward left in
 * image_buffer.  The reference stores final_T per pixel for its backward (forward.cu:373) and returns no such
 * image: its rasterizer hands out colour, radii and depth only (diff_gaussian_rasterization/__init__.py:98).
 * It is what normalises the depth image (forward.cu:359 has no background term), what a foreground mask is
 * compared with, and what compositing over another background needs.  Pixels of tiles with an empty list, and
 * every pixel when num_rendered == 0, give 0.  out_alpha: width * height floats on the device.  One streaming
 * launch on `stream`.
 * Status: GS4D_ERR_ARG for width <= 0, height <= 0 or a NULL pointer. */
int gs4d_alpha_image(int width, int height, const char *image_buffer, float *out_alpha, void *stream);

/* gs4d_backward_depth with a gradient for the alpha image of gs4d_alpha_image as well (no reference
 * counterpart; opt-in).  dL_ddepth and dL_dalpha (H * W floats each) may each be NULL: "no such gradient".
 * Both NULL is gs4d_backward_ex, dL_dalpha == NULL is gs4d_backward_depth, bit for bit; with dL_ddepth == NULL
 * the colour-only instantiations of the three stages run.  Since d(1 - T_final)/dalpha_i = T_final / (1 - alpha_i),
 * the factor the reference's background term already carries (backward.cu:531-534), dL_dalpha enters as the
 * start value of the reverse walk's running sum, bg . dL_dpix - dL_dalpha, and nowhere else: it reaches
 * dL_dopacity, dL_dmean2D and dL_dconic (hence dL_dmean3D, dL_dcov3D, dL_dscale, dL_drot); dL_dcolor and
 * dL_dsh receive nothing from it.  Results are bitwise repeatable.
 * Status as gs4d_backward_depth: GS4D_OK at once for P == 0; GS4D_ERR_ARG for P < 0, R < 0 or a NULL dL_dpix. */
int gs4d_backward_aux(int P, int D, int M, int R, const float *background, int width, int height,
                      const float *means3D, const float *shs, const float *colors_precomp, const float *scales,
                      float scale_modifier, const float *rotations, const float *cov3D_precomp,
                      const float *viewmatrix, const float *projmatrix, const float *campos, float tan_fovx,
                      float tan_fovy, const int *radii, char *geom_buffer, char *binning_buffer, char *image_buffer,
                      const float *dL_dpix, const float *dL_ddepth, const float *dL_dalpha, float *dL_dmean2D,
                      float *dL_dconic, float *dL_dopacity, float *dL_dcolor, float *dL_dmean3D, float *dL_dcov3D,
                      float *dL_dsh, float *dL_dscale, float *dL_drot, gs4d_alloc_fn scratch_alloc, void *scratch_ctx,
                      int debug, void *stream, int view_transposed);

/* gs4d_backward_aux that also returns the absolute screen-space gradient (AbsGS; gsplat's `absgrad`; no reference
 * counterpart; opt-in), the densification signal that does not cancel.  dL_dmean2D is the SIGNED sum over pixels of
 * each pixel's pull on the 2-D mean (backward.cu:541-546), so a large blurry Gaussian pulled left by half of its
 * pixels and right by the other half gets ~0 and is never split.  abs_dmean2D (P x 3 floats, device) receives, in
 * dL_dmean2D's units,
 *     abs_dmean2D[3 i + 0] = width / 2  * sum_p | dL/dG_p * dG/ddelx_p |
 *     abs_dmean2D[3 i + 1] = height / 2 * sum_p | dL/dG_p * dG/ddely_p |
 *     abs_dmean2D[3 i + 2] = 0
 * over the pixels p where the backward blends Gaussian i (the contributor, 1/255, power > 0 and 0.99-cap rules as in
 * gs4d_backward_ex; dL/dalpha includes whatever the call back-propagates: colour, and depth / alpha when given).  A
 * skipped pixel adds an exact 0; a Gaussian without instances or with radii == 0 gets exact zeros; every row is
 * written.  dL_ddepth and dL_dalpha may each be NULL as in gs4d_backward_aux.  Every other output is bit for bit
 * what gs4d_backward_ex / _depth / _aux give for the same inputs, and abs_dmean2D is bitwise repeatable (no float
 * atomics: the sums ride the fixed-order reduction of the other gradients).
 * Layout note: the 48-byte per-instance gradient record the reverse walk stores (12 floats: nine gradient sums,
 * float 9 = W3 of the depth gradient, floats 10 and 11 = these two absolute sums) is now full; a further
 * per-instance value needs a wider record.
 * Status as gs4d_backward_aux, and GS4D_ERR_ARG for a NULL abs_dmean2D (also when P == 0). */
int gs4d_backward_absgrad(int P, int D, int M, int R, const float *background, int width, int height,
                          const float *means3D, const float *shs, const float *colors_precomp, const float *scales,
                          float scale_modifier, const float *rotations, const float *cov3D_precomp,
                          const float *viewmatrix, const float *projmatrix, const float *campos, float tan_fovx,
                          float tan_fovy, const int *radii, char *geom_buffer, char *binning_buffer,
                          char *image_buffer, const float *dL_dpix, const float *dL_ddepth, const float *dL_dalpha,
                          float *dL_dmean2D, float *dL_dconic, float *dL_dopacity, float *dL_dcolor, float *dL_dmean3D,
                          float *dL_dcov3D, float *dL_dsh, float *dL_dscale, float *dL_drot, float *abs_dmean2D,
                          gs4d_alloc_fn scratch_alloc, void *scratch_ctx, int debug, void *stream,
                          int view_transposed);

/* Antialiased rasterization (Mip-Splatting's 2-D filter; the `antialiasing` switch of the current Inria
 * rasterizer, gsplat's rasterize_mode="antialiased"; no reference counterpart; opt-in).  The forward dilates every
 * projected covariance by 0.3 px^2 (forward.cu:110-111) and leaves the opacity, so a splat below a pixel deposits
 * more energy than it holds.  With (a0, b, c0) the projected covariance before the low-pass, a = a0 + 0.3,
 * c = c0 + 0.3:
 *     D0 = a0 c0 - b^2    D1 = a c - b^2    r = D0 / D1    s = sqrt(max(2.5e-5, r))    o_eff = o s
 * gs4d_forward_aa is gs4d_forward_ex plus `antialiasing`: non-zero blends with o_eff in place of o.  What changes:
 * the opacity the exact tile culling, the blend and (later) the render-level gradients read.  What does not: the
 * conic, radii, the tile rectangles and *num_rendered, which stay those of the dilated covariance.
 * antialiasing = 0 gives gs4d_forward_ex's bits. */
int gs4d_forward_aa(gs4d_alloc_fn geometry_alloc, void *geometry_ctx, gs4d_alloc_fn binning_alloc, void *binning_ctx,
                    gs4d_alloc_fn image_alloc, void *image_ctx, int P, int D, int M, const float *background,
                    int width, int height, const float *means3D, const float *shs, const float *colors_precomp,
                    const float *opacities, const float *scales, float scale_modifier, const float *rotations,
                    const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix,
                    const float *cam_pos, float tan_fovx, float tan_fovy, int prefiltered, float *out_color,
                    float *out_depth, int *radii, int debug, void *stream, int *num_rendered, int view_transposed,
                    int antialiasing);

/* The backward of gs4d_forward_aa: gs4d_backward_absgrad's arguments, then the forward's `opacities` (P floats, the
 * raw o) and `antialiasing`.  dL_ddepth, dL_dalpha and abs_dmean2D may each be NULL ("off"), so the one entry
 * serves every combination of the opt-ins.  With antialiasing != 0 (the matching forward's value) and
 * g = dL/do_eff, what the other entries return as dL_dopacity:
 *     dL_dopacity = g s        dL/ds = g o        dL/dr = r <= 2.5e-5 ? 0 : dL/ds / (2 s)
 *     dr/da0 = (c0 D1 - D0 c) / D1^2    dr/dc0 = (a0 D1 - D0 a) / D1^2    dr/db = 2 b (D0 - D1) / D1^2
 * and dL/dr times these joins the conic's gradient with respect to (a, b, c) (backward.cu:196-208) ahead of the chain
 * to dL_dcov3D (hence dL_dscale, dL_drot) and the covariance part of dL_dmean3D -- also where the reference's
 * denom2inv == 0 zeroes the conic's own terms.  The floor is a constant of the backward, and the forward and the
 * backward decide it by the same arithmetic.  dL_dmean2D, dL_dcolor, dL_dsh and abs_dmean2D are what the other
 * entries give for a plain forward whose opacities are o_eff.  antialiasing = 0 gives the bits of
 * gs4d_backward_ex / _depth / _aux / _absgrad for the same pointers; `opacities` is then not read.
 * Status as gs4d_backward_aux (GS4D_OK at once for P == 0), and GS4D_ERR_ARG for NULL `opacities` with
 * antialiasing != 0. */
int gs4d_backward_aa(int P, int D, int M, int R, const float *background, int width, int height,
                     const float *means3D, const float *shs, const float *colors_precomp, const float *scales,
                     float scale_modifier, const float *rotations, const float *cov3D_precomp,
                     const float *viewmatrix, const float *projmatrix, const float *campos, float tan_fovx,
                     float tan_fovy, const int *radii, char *geom_buffer, char *binning_buffer, char *image_buffer,
                     const float *dL_dpix, const float *dL_ddepth, const float *dL_dalpha, float *dL_dmean2D,
                     float *dL_dconic, float *dL_dopacity, float *dL_dcolor, float *dL_dmean3D, float *dL_dcov3D,
                     float *dL_dsh, float *dL_dscale, float *dL_drot, float *abs_dmean2D, gs4d_alloc_fn scratch_alloc,
                     void *scratch_ctx, int debug, void *stream, int view_transposed, const float *opacities,
                     int antialiasing);

/* gs4d_backward_aa plus the gradient with respect to the camera: its arguments, then dL_dcamera, 35 floats on the
 * device, all of them written: dL/dviewmatrix (16), dL/dprojmatrix (16), dL/dcampos (3), each matrix [i][j] at
 * 4 i + j of the 4x4 as the caller indexes it (with view_transposed != 0 too: the layout of the gradient does not
 * follow the input's strides).  The camera enters as t = ([m, 1] V)[:3], p_hom = [m, 1] Pm and dir = m - c, and
 * Rv = V[:3, :3]^T is the rotation of T = J Rv in cov2D = T Sigma T^t.  With p_h = [m, 1], summed over the
 * Gaussians with radii > 0 and at least one instance (the others add exact zeros):
 *     dL/dV[i][j]  += p_h[i] dL/dt[j]        j < 3; dL/dt as computeCov2D's backward forms it (backward.cu:262-264,
 *                                            the frustum clamp's zeros included), plus W3 on j = 2 with dL_ddepth
 *     dL/dV[k][b]  += sum_a dL/dT[a][k] J[a][b]    k, b < 3; dL/dT = 2 sym(dL/dcov2D) T Sigma
 *     dL/dPm[i][j] += p_h[i] dL/dp_hom[j]    dL/dp_hom = (w g.x, w g.y, 0, -(p_hom.x g.x + p_hom.y g.y) w^2),
 *                                            g = dL_dmean2D, w = 1 / (p_hom.w + 1e-7)
 *     dL/dc        -= the view-direction part of dL_dmean3D (computeColorFromSH's backward; zero without SHs)
 * Column 3 of dL/dV and column 2 of dL/dPm are zero.  Radii, rectangles, tile lists and the blend's decisions are
 * not differentiated, and the clamp holds the clamped t.x / t.y as a constant, as for dL_dmean3D.  The sum runs in
 * a fixed order without float atomics: per workgroup, then over the workgroups' rows in fp64; two calls give the
 * same bits.  The other outputs are gs4d_backward_aa's, bit for bit.  P == 0 gives 35 zeros.
 * Status as gs4d_backward_aa, and GS4D_ERR_ARG for a NULL dL_dcamera. */
int gs4d_backward_camera(int P, int D, int M, int R, const float *background, int width, int height,
                         const float *means3D, const float *shs, const float *colors_precomp, const float *scales,
                         float scale_modifier, const float *rotations, const float *cov3D_precomp,
                         const float *viewmatrix, const float *projmatrix, const float *campos, float tan_fovx,
                         float tan_fovy, const int *radii, char *geom_buffer, char *binning_buffer, char *image_buffer,
                         const float *dL_dpix, const float *dL_ddepth, const float *dL_dalpha, float *dL_dmean2D,
                         float *dL_dconic, float *dL_dopacity, float *dL_dcolor, float *dL_dmean3D, float *dL_dcov3D,
                         float *dL_dsh, float *dL_dscale, float *dL_drot, float *abs_dmean2D, gs4d_alloc_fn scratch_alloc,
                         void *scratch_ctx, int debug, void *stream, int view_transposed, const float *opacities,
                         int antialiasing, float *dL_dcamera);

/* Per-Gaussian blend-weight importance of a finished forward (no reference counterpart; opt-in).  The reference
 * forms the blend weight of every (pixel, splat) pair, alpha * T, only to multiply it into the colour
 * (forward.cu:357-358), and returns no such quantity: its rasterizer hands out colour, radii and depth only.
 * This entry reads the state a finished gs4d_forward / _ex / _aa over P Gaussians left in its three buffers, carved
 * exactly as gs4d_backward carves them, and replays the blend walk.  For Gaussian i, over the pixels p where the
 * forward blended it, w_ip = alpha_ip T_ip under the forward's own rules (pixels inside the image, alpha >= 1/255,
 * power <= 0 for a conic that is not positive definite, the 0.99 cap, and the splat that would drop T below 1e-4
 * not blended with the pixel retired, forward.cu:330-366); after gs4d_forward_aa the geometry state holds the
 * compensated opacity, so the weights are the antialiased forward's.
 *   weight_sum[i]  = sum_p w_ip    (LightGaussian's / Mini-Splatting's importance)
 *   weight_max[i]  = max_p w_ip    (RadSplat's pruning score)
 *   pixel_count[i] = #{p : i blends into p}    (LightGaussian's hit count)
 * Every row of the three outputs (P each, device) is written; a Gaussian with radii == 0, or with no instance that
 * survived the exact culling, gets exact zeros, and num_rendered == 0 writes P rows of zeros.  Every w_ip is bit
 * for bit the value the forward multiplied into the colour, so weight_max and pixel_count are exact statements
 * about the forward that ran.  weight_sum is summed in a fixed order -- within a wave, then per emission slot,
 * then over a Gaussian's consecutive slots -- without float atomics: two calls give the same bits.  Nothing
 * synchronises; all launches go to `stream`; the forward's buffers and outputs are left as they are.  The scratch
 * (per-slot records) comes from scratch_alloc and must stay valid until the stream has run the launches.
 * Status: GS4D_OK at once for P == 0; GS4D_ERR_ARG (message beginning "importance:") for P < 0, an empty image,
 * num_rendered < 0, or with P > 0 a NULL buffer (binning_buffer may be NULL when num_rendered == 0), output or
 * allocator; GS4D_ERR_ALLOC when scratch_alloc returns NULL. */
int gs4d_importance(int P, int width, int height, int num_rendered,
                    const char *geometry_buffer, const char *binning_buffer, const char *image_buffer,
                    float *weight_sum, float *weight_max, int32_t *pixel_count,
                    gs4d_alloc_fn scratch_alloc, void *scratch_ctx, void *stream);

/* N-channel feature rendering over a finished forward (no reference counterpart; opt-in).  `features` is P x C
 * fp32 (device, contiguous, any sign), C >= 1.  gs4d_features_forward reads the state a finished gs4d_forward / _ex /
 * _aa left in its three buffers (carved as gs4d_importance carves them), replays the blend walk and writes
 *   out_image[c][p] = sum_i w_ip features[i][c]      (C x height x width)
 * with w_ip = alpha_ip T_ip the forward's own weights under the forward's own rules (see gs4d_importance); after
 * gs4d_forward_aa they are the antialiased forward's.  There is no background term and no normalisation.  A channel
 * is accumulated as the forward accumulates a colour channel (fma(f, w, acc) in list order), so it is bit for bit
 * the colour the forward blends for colors_precomp = that column over a zero background.  The walk takes
 * gs4d_feature_chunk() channels at a time (chunks are a grid dimension) and reads the rows in place: it takes no
 * scratch, and scratch_alloc / scratch_ctx are not called (they may be NULL).  num_rendered == 0 writes a zero image.
 *
 * gs4d_features_backward takes the forward's geometry inputs and camera as gs4d_backward_aa does, plus `features`
 * and dL_dfeature_image (C x height x width), and writes
 *   dL_dfeatures[i][c] = sum_p w_ip dL_dfeature_image[c][p]      (P x C, every element)
 * and, through dL/dalpha_ip = sum_c dL/dF_c(p) (T_ip f_ic - S_ipc / (1 - alpha_ip)), S_ipc = sum_{j>i} w_jp f_jc,
 * and the chain of gs4d_backward (the 0.99 cap and, with `antialiasing`, the factor's gradient included), the
 * geometry gradients dL_dmean2D (P x 3), dL_dopacity (P), dL_dmean3D (P x 3), dL_dcov3D (P x 6), dL_dscale (P x 3)
 * and dL_drot (P x 4), every element.  A NULL dL_dmean2D asks for dL_dfeatures alone: the geometry records, their
 * reduction and the per-Gaussian stage are skipped and no geometry output is touched.  `radii` may be NULL (the
 * forward's internal radii).  Sums run in a fixed order without float atomics (per wave, per emission slot, then a
 * Gaussian's slots in order; several chunks add their geometry terms per instance in ascending chunk order): two
 * calls give the same bits.  Nothing synchronises; all launches go to `stream`; the forward's buffers are left as
 * they are.  The scratch (per-instance records: gs4d_feature_chunk() + 12 floats each, whatever C) comes from
 * scratch_alloc and must stay valid until the stream has run the launches.
 * Status (both): GS4D_OK at once for P == 0; GS4D_ERR_ARG (message beginning "features:") for C < 1, P < 0,
 * num_rendered < 0, an empty image, or with P > 0 a NULL buffer (binning_buffer may be NULL when num_rendered == 0),
 * input or required output; the backward also for a NULL allocator, and GS4D_ERR_ALLOC when it returns NULL. */
int gs4d_feature_chunk(void);
int gs4d_features_forward(int P, int C, int width, int height, int num_rendered, const char *geometry_buffer,
                          const char *binning_buffer, const char *image_buffer, const float *features,
                          float *out_image, gs4d_alloc_fn scratch_alloc, void *scratch_ctx, void *stream);
int gs4d_features_backward(int P, int C, int num_rendered, int width, int height, const float *means3D,
                           const float *scales, float scale_modifier, const float *rotations,
                           const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix,
                           float tan_fovx, float tan_fovy, const int *radii, char *geom_buffer, char *binning_buffer,
                           char *image_buffer, const float *features, const float *dL_dfeature_image,
                           float *dL_dfeatures, float *dL_dmean2D, float *dL_dopacity, float *dL_dmean3D,
                           float *dL_dcov3D, float *dL_dscale, float *dL_drot, gs4d_alloc_fn scratch_alloc,
                           void *scratch_ctx, void *stream, int view_transposed, const float *opacities,
                           int antialiasing);

/* Replaces SimpleKNN::knn(submodules/simple-knn/simple_knn.h:14-20, simple_knn.cu:187-223), the
 * native layer behind simple_knn._C.distCUDA2 (spatial.cu:15-25, ext.cpp:15-16), which
 * scene/gaussian_model.py:148-149 uses to initialise the Gaussian scales.
 * points: P x 3 fp32 (device, contiguous).  mean_dists[i] = mean of the squared distances from point i
 * to its 3 nearest other points (the reference's Morton-box search, which prunes but never changes the
 * result).  The scratch buffer comes from scratch_alloc and must stay valid until the stream has run
 * the launches.  P == 0 is a no-op. */
int gs4d_knn_mean_dist(int P, const float *points, float *mean_dists, gs4d_alloc_fn scratch_alloc, void *scratch_ctx,
                       void *stream);

/* The exact K-nearest-neighbour graph of a cloud, with its transpose (no reference counterpart; opt-in: the
 * local-isometry regulariser of gs4d_train.h reads it).  The search is gs4d_knn_mean_dist's, keeping the neighbours.
 * points: P x 3 fp32 (device, contiguous); K in 1..16.
 *   nbr_idx[i K + k], nbr_dist2[i K + k]: the K nearest OTHER points of point i (self excluded by index) and their
 *     squared distances (dx dx + dy dy) + dz dz in fp32 without contraction, ascending by (distance, index): equal
 *     distances go to the lower index.  Slots beyond min(K, P - 1) hold -1 and FLT_MAX.
 *   Edge e = i K + k has target nbr_idx[e].  in_edge[in_start[t] .. in_start[t + 1]) are the ids of the valid
 *     edges whose target is t, ascending; in_start has P + 1 entries, in_edge P K, those past in_start[P] are -1.
 * Nothing synchronises; every launch goes to `stream`; the scratch must stay valid until the stream has run them.
 * The result is a function of the points alone: no atomic decides an order, two calls give the same bits.
 * Status: GS4D_OK at once for P == 0; GS4D_ERR_ARG (message beginning "knn_graph:") for K outside 1..16, P < 0,
 * P K >= 2^30, or with P > 0 a NULL pointer or a NULL allocator, all before the allocator is asked; GS4D_ERR_ALLOC
 * when it returns NULL. */
int gs4d_knn_graph(int P, int K, const float *points, int32_t *nbr_idx, float *nbr_dist2, int32_t *in_start,
                   int32_t *in_edge, gs4d_alloc_fn scratch_alloc, void *scratch_ctx, void *stream);

/* Instant4D grid pruning: replaces the Open3D voxel_down_sample call of utils/grid_pruning.py:16-41, which
 * scene/__init__.py:106-119 runs on the initial cloud in front of create_from_pcd (and so in front of
 * gs4d_knn_mean_dist).  Semantics (Open3D's PointCloud::VoxelDownSample, with a defined row order):
 *   - origin = per-axis minimum of the points (as fp64) - voxel_size / 2;
 *   - voxel index per axis = floor((double(p) - origin) / voxel_size): fp64, a true division, no contraction,
 *     so it equals numpy's for the same inputs;
 *   - one output row per occupied voxel: the arithmetic mean of that voxel's points (and colours), summed in
 *     fp64 in a fixed order and rounded once to fp32; out_counts[row] = how many points fell in;
 *   - rows ascend in the linear index (iz * ny + iy) * nx + ix, n* = largest index + 1 (Open3D's order is its
 *     hash map's, i.e. unspecified);
 *   - normals are not produced (create_from_pcd ignores them).
 * points / colors: N x 3 fp32 device arrays; colors may be NULL, and out_colors is NULL exactly when it is.
 * out_points / out_colors (N x 3) and out_counts (N int32, may be NULL) have room for N rows; the first
 * *num_voxels = M rows are written.  Results are bitwise repeatable (no floating-point atomics).
 * The call synchronises `stream` twice -- once to read the six bounds, once to read M -- as gs4d_forward does
 * once for num_rendered; the scratch buffer may be released when it returns.
 * GS4D_ERR_ARG (gs4d_last_error() begins "voxel_downsample:"), before any launch: N < 0 or N >= 2^30,
 * voxel_size not finite or <= 0, a NULL required pointer or allocator, colors / out_colors not both set or
 * both NULL; after the bounds readback: a NaN or infinite coordinate, an axis of 2^21 voxels or more.
 * N == 0 is a successful no-op with M = 0. */
int gs4d_voxel_downsample(int N, const float *points, const float *colors, double voxel_size, float *out_points,
                          float *out_colors, int32_t *out_counts, int *num_voxels, gs4d_alloc_fn scratch_alloc,
                          void *scratch_ctx, void *stream);

/* Diagnostic for the parity tests (no reference counterpart): for n (Gaussian, pixel) pairs, o G (the
 * blend's alpha before the 0.99 cap) and the base-2 exponent log2(G), evaluated by the exact arithmetic
 * of the blend kernels from the packed splat records a gs4d_forward left in geometry_buffer (P Gaussians,
 * a width x height image).  gid/px/py: n int32 device arrays; og/pw: n fp32 device outputs. */
int gs4d_debug_pair_alpha(int P, int width, int height, const char *geometry_buffer, int n, const int *gid,
                          const int *px, const int *py, float *og, float *pw, void *stream);

/* Diagnostic for the antialiasing tests (no reference counterpart): out[i] = the opacity the blend reads for
 * Gaussian i (conic_opacity.w of the geometry state a forward over P Gaussians left in geometry_buffer): o after a
 * plain forward, o_eff = o s after gs4d_forward_aa with antialiasing.  out: P floats on the device.  Rows of
 * Gaussians the forward culled (radii == 0) are unspecified.  GS4D_ERR_ARG for P < 0 or a NULL pointer with P > 0. */
int gs4d_debug_effective_opacity(int P, const char *geometry_buffer, float *out, void *stream);

/* Diagnostic for the tile-list tests (no reference counterpart; read-only): the per-tile instance lists a finished
 * gs4d_forward over P > 0 Gaussians and a width x height image left in its three buffers, in render order (by tile,
 * then depth bits, then Gaussian id).  The buffers are carved exactly as gs4d_backward carves them, num_rendered being
 * the forward's.  With T = ceil(width / 16) * ceil(height / 16) tiles, all outputs on the device:
 *   ranges     2 T uint32: tile t's list is positions [ranges[2 t], ranges[2 t + 1]); an empty tile has (0, 0)
 *   order      T uint32: the blend kernels' workgroup -> tile map (longest list first)
 *   n_emitted  1 uint32: L' <= num_rendered, the (tile, splat) pairs that survived the exact tile culling
 *   gid, reach, slot (uint32) and depth (float), num_rendered elements each, of which the first L' are written:
 *     for list position i the Gaussian id, its half-tile reach bits (bit h: rows 8 h .. 8 h + 7 of the tile), its
 *     emission slot (where the backward writes the pair's gradient record) and the view depth the sort read.
 *     A position whose slot or id is out of range (buffers that are not this forward's) reads gid = 0xFFFFFFFF.
 * num_rendered == 0: ranges and order are copied, n_emitted = 0, nothing else is touched (the lists may be NULL).
 * GS4D_ERR_ARG (gs4d_last_error() begins "debug_tile_lists:") for P <= 0, an empty image, num_rendered < 0 or a
 * NULL pointer that is needed. */
int gs4d_debug_tile_lists(int P, int width, int height, int num_rendered, const char *geometry_buffer,
                          const char *binning_buffer, const char *image_buffer, uint32_t *ranges, uint32_t *order,
                          uint32_t *n_emitted, uint32_t *gid, uint32_t *reach, uint32_t *slot, float *depth,
                          void *stream);

/* Diagnostic for the blend backward's pair reduction (no reference counterpart): n pairs of splats, one wave
 * each, reduce given per-lane partial sums to their two 12-float records, once as the blend kernel does (column
 * sums through LDS) and once by permlane swaps (the earlier form, kept for this comparison): the two must agree
 * to the bit.  in: n x 20 x 64 fp32 on the device, value k of lane l of pair p at (20 p + k) 64 + l, with
 * k = 0-5 splat a's (u0, u1, u2, w0, w1, w2), 6-11 splat b's, 12-13 W3 of a and b, 14-17 (a.AX, a.AY, b.AX, b.AY),
 * 18-19 the lanes' dx of a and b.  depth / abs select the instantiation (W3 and the absolute sums are read only
 * by theirs).  out_lds / out_permlane: n x 24 fp32, a's record then b's; floats the instantiation does not
 * produce are 0. */
int gs4d_debug_wave_sum(int n, const float *in, int depth, int abs, float *out_lds, float *out_permlane,
                        void *stream);

/* How many workgroups (one wave each) of the blend backward's (depth, abs) instantiation the runtime keeps
 * resident on one CU, by its registers and LDS: 4 waves per SIMD are 16, 3 are 12. */
int gs4d_debug_backward_occupancy(int depth, int abs, int *workgroups_per_cu);

/* Human-readable message for the last error on this thread (never NULL). */
const char *gs4d_last_error(void);

/* Library version string, e.g. "gs4d 0.1.0 gfx950". */
const char *gs4d_version(void);

/* Per-kernel timing of the most recent gs4d_forward / gs4d_backward on this thread, recorded with
 * hipEvents on the launch stream when profiling is enabled (bench.py).  names[i] / ms[i] for
 * i < *count; returns the number of entries.  enabled >= 2 launches the two blend kernels (render,
 * render_backward) that many times back to back and reports their per-launch average (an entry
 * "<name>_pre" then holds the time up to that stage). */
void gs4d_set_profiling(int enabled);
int gs4d_last_timings(const char **names, float *ms, int max_entries);

#ifdef __cplusplus
}
#endif

#endif /* GS4D_H_INCLUDED */
