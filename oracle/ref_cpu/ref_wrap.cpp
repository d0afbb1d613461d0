/* extern "C" entries over the reference's CudaRasterizer::Rasterizer, compiled for the host (cuda_on_cpu.h).
 * The three state chunks live in std::vector<char>s behind the std::function allocators that the reference's
 * forward asks for; the export reads them back through the reference's own fromChunk layouts. */
#include "cuda_on_cpu.h"

#include "rasterizer.h"
#include "rasterizer_impl.h"

namespace {
struct State {
    std::vector<char> geom, binning, image;
    int P, W, H, num_rendered;
};
std::function<char *(size_t)> allocator(std::vector<char> &v) {
    return [&v](size_t n) { v.assign(n, 0); return v.data(); };
}
}

extern "C" {

void *gs4d_ref_forward(int P, int D, int M, const float *background, int W, int H, const float *means3D,
                       const float *shs, const float *colors_precomp, const float *opacities, const float *scales,
                       float scale_modifier, const float *rotations, const float *cov3D_precomp,
                       const float *viewmatrix, const float *projmatrix, const float *campos, float tan_fovx,
                       float tan_fovy, float *out_color, float *out_depth, int *radii, int *num_rendered) {
    State *s = new State;
    s->P = P; s->W = W; s->H = H;
    s->num_rendered = CudaRasterizer::Rasterizer::forward(
        allocator(s->geom), allocator(s->binning), allocator(s->image), P, D, M, background, W, H, means3D, shs,
        colors_precomp, opacities, scales, scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, campos,
        tan_fovx, tan_fovy, /*prefiltered=*/false, out_color, out_depth, radii, /*debug=*/false);
    *num_rendered = s->num_rendered;
    return s;
}

/* every output starts zeroed (the kernels accumulate into them) */
void gs4d_ref_backward(void *state, int D, int M, const float *background, const float *means3D, const float *shs,
                       const float *colors_precomp, const float *scales, float scale_modifier, const float *rotations,
                       const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix,
                       const float *campos, float tan_fovx, float tan_fovy, const int *radii, const float *dL_dpix,
                       float *dL_dmean2D, float *dL_dconic, float *dL_dopacity, float *dL_dcolor, float *dL_dmean3D,
                       float *dL_dcov3D, float *dL_dsh, float *dL_dscale, float *dL_drot) {
    State *s = (State *)state;
    CudaRasterizer::Rasterizer::backward(
        s->P, D, M, s->num_rendered, background, s->W, s->H, means3D, shs, colors_precomp, scales, scale_modifier,
        rotations, cov3D_precomp, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, radii, s->geom.data(),
        s->binning.data(), s->image.data(), dL_dpix, dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_dmean3D,
        dL_dcov3D, dL_dsh, dL_dscale, dL_drot, /*debug=*/false);
}

/* clamped: bit c set where channel c was clamped; ranges: one (start, end) pair per tile */
void gs4d_ref_state_export(void *state, float *depths, float *means2D, float *cov3D, float *conic_opacity, float *rgb,
                           uint8_t *clamped, uint32_t *tiles_touched, uint32_t *point_list, uint32_t *ranges,
                           float *accum_alpha, uint32_t *n_contrib) {
    State *s = (State *)state;
    const size_t P = s->P, N = (size_t)s->W * s->H, L = s->num_rendered;
    const size_t tiles = (size_t)((s->W + 15) / 16) * ((s->H + 15) / 16);
    char *chunk = s->geom.data();
    CudaRasterizer::GeometryState g = CudaRasterizer::GeometryState::fromChunk(chunk, P);
    chunk = s->binning.data();
    CudaRasterizer::BinningState b = CudaRasterizer::BinningState::fromChunk(chunk, L);
    chunk = s->image.data();
    CudaRasterizer::ImageState im = CudaRasterizer::ImageState::fromChunk(chunk, N);
    memcpy(depths, g.depths, 4 * P);
    memcpy(means2D, g.means2D, 8 * P);
    memcpy(cov3D, g.cov3D, 24 * P);
    memcpy(conic_opacity, g.conic_opacity, 16 * P);
    memcpy(rgb, g.rgb, 12 * P);
    for (size_t i = 0; i < P; i++)
        clamped[i] = (uint8_t)((g.clamped[3 * i] ? 1 : 0) | (g.clamped[3 * i + 1] ? 2 : 0) | (g.clamped[3 * i + 2] ? 4 : 0));
    memcpy(tiles_touched, g.tiles_touched, 4 * P);
    memcpy(point_list, b.point_list, 4 * L);
    memcpy(ranges, im.ranges, 8 * tiles);
    memcpy(accum_alpha, im.accum_alpha, 4 * N);
    memcpy(n_contrib, im.n_contrib, 4 * N);
}

void gs4d_ref_free(void *state) { delete (State *)state; }

void gs4d_ref_mark_visible(int P, const float *means3D, const float *viewmatrix, const float *projmatrix,
                           uint8_t *present) {
    static_assert(sizeof(bool) == 1, "present is written as bool");
    CudaRasterizer::Rasterizer::markVisible(P, (float *)means3D, (float *)viewmatrix, (float *)projmatrix,
                                            (bool *)present);
}

}
