// torch_glue.cpp -- the `_C` extension module: PyTorch-ROCm tensors -> libgs4d C ABI.
//
// Mirrors the reference's torch glue rasterize_points.cu:27-219 and its pybind table ext.cpp:15-18:
// same function names, positional arguments, return tuples and error behaviour (RuntimeError for
// AT_ERROR / runtime_error paths).  Differences: launches go to the *current* HIP stream instead of
// the legacy default stream; inputs must live on the GPU (there is no CPU fallback in the product
// path -- CPU tensors raise); gradient outputs are allocated uninitialised because libgs4d writes
// every element.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <c10/hip/HIPGuard.h>
#include <torch/extension.h>

#include <algorithm>
#include <functional>
#include <string>
#include <tuple>

#include "../../include/gs4d.h"

namespace {

struct Resizer {
    torch::Tensor *t;
};
// rasterize_points.cu:27-33 resizeFunctional as a C callback.  The buffers start empty and are sized once per
// call, so a fresh allocation stands in for resize_ (same result; resize_ took ~8 us of host time per buffer)
char *resize_cb(void *ctx, size_t n) {
    auto *r = static_cast<Resizer *>(ctx);
    if (r->t->numel() == 0)
        *r->t = torch::empty({(long long)n}, r->t->options());
    else
        r->t->resize_({(long long)n});
    return reinterpret_cast<char *>(r->t->data_ptr());
}

void check_status(int st, const char *what) {
    if (st != GS4D_OK) throw std::runtime_error(std::string(what) + ": " + gs4d_last_error());
}

// Empty tensor -> nullptr (the reference's convention, rasterize_points.cu:95-106).
// Non-empty tensors must be float32 on the current HIP device; returns a contiguous, 16-byte
// aligned tensor that the caller keeps alive for the duration of the call.
torch::Tensor prep(const torch::Tensor &t, const char *name, const torch::Device &dev) {
    if (t.numel() == 0) return t;
    if (!t.is_cuda()) throw std::runtime_error(std::string(name) + " must be a HIP (GPU) tensor; the MI355X rasterizer has no CPU path");
    if (t.device() != dev) throw std::runtime_error(std::string(name) + " is on a different device than means3D");
    if (t.scalar_type() != torch::kFloat32) throw std::runtime_error(std::string(name) + " must be float32");
    torch::Tensor c = t.contiguous();
    if ((reinterpret_cast<uintptr_t>(c.data_ptr()) & 15) != 0) c = c.clone();
    return c;
}
const float *fptr(const torch::Tensor &t) { return t.numel() ? t.data_ptr<float>() : nullptr; }

// The view matrix as the reference's callers pass it: world_view_transform is a transposed 4x4 view
// (strides (1, 4)); such a matrix is read in place by the kernels (view_transposed = 1) instead of
// being copied by .contiguous().  Anything else goes through prep().
torch::Tensor prep_view(const torch::Tensor &t, const torch::Device &dev, int &transposed) {
    transposed = 0;
    if (t.numel() == 16 && t.dim() >= 2 && t.size(-1) == 4 && t.size(-2) == 4 && t.stride(-1) == 4 &&
        t.stride(-2) == 1 && t.is_cuda() && t.device() == dev && t.scalar_type() == torch::kFloat32 &&
        (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0) {
        transposed = 1;
        return t;
    }
    return prep(t, "viewmatrix", dev);
}

}  // namespace

// rasterize_points.cu:35-117; antialiasing: gs4d_forward_aa's switch (0 = the reference's forward)
using ForwardTuple = std::tuple<int, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>;
static ForwardTuple
ForwardImpl(const bool antialiasing, const torch::Tensor &background, const torch::Tensor &means3D, const torch::Tensor &colors,
                   const torch::Tensor &opacity, const torch::Tensor &scales, const torch::Tensor &rotations,
                   const float scale_modifier, const torch::Tensor &cov3D_precomp, const torch::Tensor &viewmatrix,
                   const torch::Tensor &projmatrix, const float tan_fovx, const float tan_fovy, const int image_height,
                   const int image_width, const torch::Tensor &sh, const int degree, const torch::Tensor &campos,
                   const bool prefiltered, const bool debug) {
    if (means3D.ndimension() != 2 || means3D.size(1) != 3) {
        AT_ERROR("means3D must have dimensions (num_points, 3)");
    }
    if (!means3D.is_cuda()) throw std::runtime_error("means3D must be a HIP (GPU) tensor; the MI355X rasterizer has no CPU path");
    const auto dev = means3D.device();
    c10::hip::HIPGuard guard(dev.index());
    const int P = means3D.size(0);
    const int H = image_height;
    const int W = image_width;
    auto float_opts = means3D.options().dtype(torch::kFloat32);
    auto byte_opts = means3D.options().dtype(torch::kByte);

    torch::Tensor geomBuffer = torch::empty({0}, byte_opts);
    torch::Tensor binningBuffer = torch::empty({0}, byte_opts);
    torch::Tensor imgBuffer = torch::empty({0}, byte_opts);
    torch::Tensor radii = torch::empty({P}, means3D.options().dtype(torch::kInt32));
    if (P == 0) {
        // the reference returns zero images when there is nothing to draw (forward never runs)
        return std::make_tuple(0, torch::zeros({3, H, W}, float_opts), torch::zeros({1, H, W}, float_opts), radii,
                               geomBuffer, binningBuffer, imgBuffer);
    }
    torch::Tensor out_color = torch::empty({3, H, W}, float_opts);
    torch::Tensor out_depth = torch::empty({1, H, W}, float_opts);

    int M = 0;
    if (sh.size(0) != 0) M = sh.size(1);
    auto bg = prep(background, "bg", dev), m3 = prep(means3D, "means3D", dev), col = prep(colors, "colors_precomp", dev),
         op = prep(opacity, "opacities", dev), sc = prep(scales, "scales", dev), rot = prep(rotations, "rotations", dev),
         c3 = prep(cov3D_precomp, "cov3D_precomp", dev), pm = prep(projmatrix, "projmatrix", dev),
         shc = prep(sh, "sh", dev), cp = prep(campos, "campos", dev);
    int vt = 0;
    auto vm = prep_view(viewmatrix, dev, vt);

    Resizer rg{&geomBuffer}, rb{&binningBuffer}, ri{&imgBuffer};
    hipStream_t stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
    int rendered = 0;
    int st = gs4d_forward_aa(resize_cb, &rg, resize_cb, &rb, resize_cb, &ri, P, degree, M, fptr(bg), W, H, fptr(m3),
                             fptr(shc), fptr(col), fptr(op), fptr(sc), scale_modifier, fptr(rot), fptr(c3), fptr(vm),
                             fptr(pm), fptr(cp), tan_fovx, tan_fovy, prefiltered ? 1 : 0, out_color.data_ptr<float>(),
                             out_depth.data_ptr<float>(), radii.data_ptr<int>(), debug ? 1 : 0, (void *)stream,
                             &rendered, vt, antialiasing ? 1 : 0);
    check_status(st, "rasterize_gaussians");
    return std::make_tuple(rendered, out_color, out_depth, radii, geomBuffer, binningBuffer, imgBuffer);
}

ForwardTuple
RasterizeGaussians(const torch::Tensor &background, const torch::Tensor &means3D, const torch::Tensor &colors,
                   const torch::Tensor &opacity, const torch::Tensor &scales, const torch::Tensor &rotations,
                   const float scale_modifier, const torch::Tensor &cov3D_precomp, const torch::Tensor &viewmatrix,
                   const torch::Tensor &projmatrix, const float tan_fovx, const float tan_fovy, const int image_height,
                   const int image_width, const torch::Tensor &sh, const int degree, const torch::Tensor &campos,
                   const bool prefiltered, const bool debug) {
    return ForwardImpl(false, background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                       viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                       prefiltered, debug);
}

// rasterize_gaussians' arguments, then `antialiasing`: gs4d_forward_aa (the opacity blended is o * s)
ForwardTuple
RasterizeGaussiansAA(const torch::Tensor &background, const torch::Tensor &means3D, const torch::Tensor &colors,
                     const torch::Tensor &opacity, const torch::Tensor &scales, const torch::Tensor &rotations,
                     const float scale_modifier, const torch::Tensor &cov3D_precomp, const torch::Tensor &viewmatrix,
                     const torch::Tensor &projmatrix, const float tan_fovx, const float tan_fovy,
                     const int image_height, const int image_width, const torch::Tensor &sh, const int degree,
                     const torch::Tensor &campos, const bool prefiltered, const bool debug, const bool antialiasing) {
    return ForwardImpl(antialiasing, background, means3D, colors, opacity, scales, rotations, scale_modifier,
                       cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree,
                       campos, prefiltered, debug);
}

// rasterize_points.cu:119-198; dL_dout_depth != nullptr: the depth-gradient backward (gs4d_backward_depth);
// dL_dout_alpha != nullptr: gs4d_backward_aux, where an empty tensor for either image means "no such gradient";
// opacities != nullptr: gs4d_backward_aa (the forward's raw opacities and its `antialiasing`)
using BackwardTuple = std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
                                 torch::Tensor, torch::Tensor, torch::Tensor>;
static BackwardTuple
BackwardImpl(const torch::Tensor *dL_dout_depth, const torch::Tensor *dL_dout_alpha, const torch::Tensor &background,
             const torch::Tensor &means3D, const torch::Tensor &radii,
                           const torch::Tensor &colors, const torch::Tensor &scales, const torch::Tensor &rotations,
                           const float scale_modifier, const torch::Tensor &cov3D_precomp,
                           const torch::Tensor &viewmatrix, const torch::Tensor &projmatrix, const float tan_fovx,
                           const float tan_fovy, const torch::Tensor &dL_dout_color, const torch::Tensor &sh,
                           const int degree, const torch::Tensor &campos, const torch::Tensor &geomBuffer, const int R,
                           const torch::Tensor &binningBuffer, const torch::Tensor &imageBuffer, const bool debug,
                           torch::Tensor *abs_out = nullptr, const torch::Tensor *opacities = nullptr,
             const bool antialiasing = false, torch::Tensor *cam_out = nullptr) {
    if (!means3D.is_cuda()) throw std::runtime_error("means3D must be a HIP (GPU) tensor; the MI355X rasterizer has no CPU path");
    const auto dev = means3D.device();
    c10::hip::HIPGuard guard(dev.index());
    const int P = means3D.size(0);
    const int H = dL_dout_color.size(1);
    const int W = dL_dout_color.size(2);
    int M = 0;
    if (sh.size(0) != 0) M = sh.size(1);
    auto opts = means3D.options().dtype(torch::kFloat32);
    torch::Tensor dL_dmeans3D = torch::empty({P, 3}, opts);
    torch::Tensor dL_dmeans2D = torch::empty({P, 3}, opts);
    torch::Tensor dL_dcolors = torch::empty({P, 3}, opts);
    torch::Tensor dL_dopacity = torch::empty({P, 1}, opts);
    torch::Tensor dL_dcov3D = torch::empty({P, 6}, opts);
    torch::Tensor dL_dsh = torch::empty({P, M, 3}, opts);
    torch::Tensor dL_dscales = torch::empty({P, 3}, opts);
    torch::Tensor dL_drotations = torch::empty({P, 4}, opts);
    if (abs_out) *abs_out = torch::empty({P, 3}, opts);  // gs4d_backward_absgrad writes every row
    if (cam_out) *cam_out = torch::empty({35}, opts);  // gs4d_backward_camera writes all 35 floats
    if (P != 0) {
        auto bg = prep(background, "bg", dev), m3 = prep(means3D, "means3D", dev), col = prep(colors, "colors_precomp", dev),
             sc = prep(scales, "scales", dev), rot = prep(rotations, "rotations", dev),
             c3 = prep(cov3D_precomp, "cov3D_precomp", dev), pm = prep(projmatrix, "projmatrix", dev),
             dl = prep(dL_dout_color, "grad_out_color", dev), shc = prep(sh, "sh", dev),
             cp = prep(campos, "campos", dev);
        int vt = 0;
        auto vm = prep_view(viewmatrix, dev, vt);
        torch::Tensor dd, da;
        if (dL_dout_depth && !(dL_dout_alpha && dL_dout_depth->numel() == 0)) {
            if (dL_dout_depth->numel() != (long long)H * W)
                throw std::runtime_error("grad_out_depth must have H * W elements");
            dd = prep(*dL_dout_depth, "grad_out_depth", dev);
        }
        if (dL_dout_alpha && dL_dout_alpha->numel() != 0) {
            if (dL_dout_alpha->numel() != (long long)H * W)
                throw std::runtime_error("grad_out_alpha must have H * W elements");
            da = prep(*dL_dout_alpha, "grad_out_alpha", dev);
        }
        torch::Tensor rad = radii.contiguous();
        if (rad.numel() && (rad.scalar_type() != torch::kInt32 || !rad.is_cuda()))
            throw std::runtime_error("radii must be an int32 GPU tensor");
        torch::Tensor scratch = torch::empty({0}, means3D.options().dtype(torch::kByte));
        Resizer rs{&scratch};
        hipStream_t stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
        const int *rad_ptr = rad.numel() ? rad.data_ptr<int>() : nullptr;
        char *geom = reinterpret_cast<char *>(geomBuffer.data_ptr());
        char *binning = binningBuffer.numel() ? reinterpret_cast<char *>(binningBuffer.data_ptr()) : nullptr;
        char *image = reinterpret_cast<char *>(imageBuffer.data_ptr());
        float *dsh = M ? dL_dsh.data_ptr<float>() : nullptr;
        // every entry takes the same 23 inputs, then its upstream images, the nine gradient outputs (dL_dconic is not
        // wanted), abs_dmean2D where it has one, and the same tail
        const auto head = std::make_tuple(P, degree, M, R, fptr(bg), W, H, fptr(m3), fptr(shc), fptr(col), fptr(sc),
                                          scale_modifier, fptr(rot), fptr(c3), fptr(vm), fptr(pm), fptr(cp), tan_fovx,
                                          tan_fovy, rad_ptr, geom, binning, image);
        const auto outs = std::make_tuple(dL_dmeans2D.data_ptr<float>(), (float *)nullptr, dL_dopacity.data_ptr<float>(),
                                          dL_dcolors.data_ptr<float>(), dL_dmeans3D.data_ptr<float>(),
                                          dL_dcov3D.data_ptr<float>(), dsh, dL_dscales.data_ptr<float>(),
                                          dL_drotations.data_ptr<float>());
        const auto tail = std::make_tuple(&resize_cb, (void *)&rs, debug ? 1 : 0, (void *)stream, vt);
        const float *pix = fptr(dl), *dep = dd.defined() ? fptr(dd) : nullptr, *alp = da.defined() ? fptr(da) : nullptr;
        const auto call = [&](const char *what, auto entry, auto images, auto abs_ptr) {
            check_status(std::apply(entry, std::tuple_cat(head, images, outs, abs_ptr, tail)), what);
        };
        if (cam_out) {
            if (!opacities) throw std::runtime_error("the camera-gradient backward takes the forward's opacities");
            if (antialiasing && opacities->numel() != P) throw std::runtime_error("opacities must have P elements");
            auto op = prep(*opacities, "opacities", dev);
            check_status(std::apply(gs4d_backward_camera,
                                    std::tuple_cat(head, std::make_tuple(pix, dep, alp), outs,
                                                   std::make_tuple(abs_out ? abs_out->data_ptr<float>() : (float *)nullptr),
                                                   tail, std::make_tuple(fptr(op), antialiasing ? 1 : 0,
                                                                         cam_out->data_ptr<float>()))),
                         "rasterize_gaussians_backward_camera");
        } else if (opacities) {
            if (antialiasing && opacities->numel() != P) throw std::runtime_error("opacities must have P elements");
            auto op = prep(*opacities, "opacities", dev);
            check_status(std::apply(gs4d_backward_aa,
                                    std::tuple_cat(head, std::make_tuple(pix, dep, alp), outs,
                                                   std::make_tuple(abs_out ? abs_out->data_ptr<float>() : (float *)nullptr),
                                                   tail, std::make_tuple(fptr(op), antialiasing ? 1 : 0))),
                         "rasterize_gaussians_backward_aa");
        } else if (abs_out)
            call("rasterize_gaussians_backward_absgrad", gs4d_backward_absgrad, std::make_tuple(pix, dep, alp),
                 std::make_tuple(abs_out->data_ptr<float>()));
        else if (dL_dout_alpha)
            call("rasterize_gaussians_backward_aux", gs4d_backward_aux, std::make_tuple(pix, dep, alp), std::tuple<>());
        else if (dL_dout_depth)
            call("rasterize_gaussians_backward_depth", gs4d_backward_depth, std::make_tuple(pix, dep), std::tuple<>());
        else
            call("rasterize_gaussians_backward", gs4d_backward_ex, std::make_tuple(pix), std::tuple<>());
    }
    if (P == 0 && cam_out) {  // no Gaussian: the entry still owes the 35 zeros
        hipStream_t stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
        check_status(gs4d_backward_camera(0, degree, M, R, nullptr, W, H, nullptr, nullptr, nullptr, nullptr,
                                          scale_modifier, nullptr, nullptr, nullptr, nullptr, nullptr, tan_fovx, tan_fovy,
                                          nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                          nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                          nullptr, debug ? 1 : 0, (void *)stream, 0, nullptr, antialiasing ? 1 : 0,
                                          cam_out->data_ptr<float>()),
                     "rasterize_gaussians_backward_camera");
    }
    return std::make_tuple(dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales,
                           dL_drotations);
}

BackwardTuple
RasterizeGaussiansBackward(const torch::Tensor &background, const torch::Tensor &means3D, const torch::Tensor &radii,
                           const torch::Tensor &colors, const torch::Tensor &scales, const torch::Tensor &rotations,
                           const float scale_modifier, const torch::Tensor &cov3D_precomp,
                           const torch::Tensor &viewmatrix, const torch::Tensor &projmatrix, const float tan_fovx,
                           const float tan_fovy, const torch::Tensor &dL_dout_color, const torch::Tensor &sh,
                           const int degree, const torch::Tensor &campos, const torch::Tensor &geomBuffer, const int R,
                           const torch::Tensor &binningBuffer, const torch::Tensor &imageBuffer, const bool debug) {
    return BackwardImpl(nullptr, nullptr, background, means3D, radii, colors, scales, rotations, scale_modifier,
                        cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh, degree, campos,
                        geomBuffer, R, binningBuffer, imageBuffer, debug);
}

// the same with the depth image's gradient (1, H, W) or (H, W) after dL_dout_color: gs4d_backward_depth
BackwardTuple
RasterizeGaussiansBackwardDepth(const torch::Tensor &background, const torch::Tensor &means3D,
                                const torch::Tensor &radii, const torch::Tensor &colors, const torch::Tensor &scales,
                                const torch::Tensor &rotations, const float scale_modifier,
                                const torch::Tensor &cov3D_precomp, const torch::Tensor &viewmatrix,
                                const torch::Tensor &projmatrix, const float tan_fovx, const float tan_fovy,
                                const torch::Tensor &dL_dout_color, const torch::Tensor &dL_dout_depth,
                                const torch::Tensor &sh, const int degree, const torch::Tensor &campos,
                                const torch::Tensor &geomBuffer, const int R, const torch::Tensor &binningBuffer,
                                const torch::Tensor &imageBuffer, const bool debug) {
    return BackwardImpl(&dL_dout_depth, nullptr, background, means3D, radii, colors, scales, rotations, scale_modifier,
                        cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh, degree, campos,
                        geomBuffer, R, binningBuffer, imageBuffer, debug);
}

// the same with the alpha image's gradient after the depth image's: gs4d_backward_aux.  An empty tensor for
// either means "none" (both empty: the colour-only backward's bits)
BackwardTuple
RasterizeGaussiansBackwardAux(const torch::Tensor &background, const torch::Tensor &means3D,
                              const torch::Tensor &radii, const torch::Tensor &colors, const torch::Tensor &scales,
                              const torch::Tensor &rotations, const float scale_modifier,
                              const torch::Tensor &cov3D_precomp, const torch::Tensor &viewmatrix,
                              const torch::Tensor &projmatrix, const float tan_fovx, const float tan_fovy,
                              const torch::Tensor &dL_dout_color, const torch::Tensor &dL_dout_depth,
                              const torch::Tensor &dL_dout_alpha, const torch::Tensor &sh, const int degree,
                              const torch::Tensor &campos, const torch::Tensor &geomBuffer, const int R,
                              const torch::Tensor &binningBuffer, const torch::Tensor &imageBuffer, const bool debug) {
    return BackwardImpl(&dL_dout_depth, &dL_dout_alpha, background, means3D, radii, colors, scales, rotations,
                        scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh,
                        degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug);
}

// rasterize_gaussians_backward_aux's arguments; returns its tuple plus the (P, 3) absolute screen-space gradient
// (gs4d_backward_absgrad): sums over pixels of |per-pixel mean2D term|, in dL_dmeans2D's units
using AbsgradTuple = std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
                                torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>;
AbsgradTuple
RasterizeGaussiansBackwardAbsgrad(const torch::Tensor &background, const torch::Tensor &means3D,
                                  const torch::Tensor &radii, const torch::Tensor &colors, const torch::Tensor &scales,
                                  const torch::Tensor &rotations, const float scale_modifier,
                                  const torch::Tensor &cov3D_precomp, const torch::Tensor &viewmatrix,
                                  const torch::Tensor &projmatrix, const float tan_fovx, const float tan_fovy,
                                  const torch::Tensor &dL_dout_color, const torch::Tensor &dL_dout_depth,
                                  const torch::Tensor &dL_dout_alpha, const torch::Tensor &sh, const int degree,
                                  const torch::Tensor &campos, const torch::Tensor &geomBuffer, const int R,
                                  const torch::Tensor &binningBuffer, const torch::Tensor &imageBuffer,
                                  const bool debug) {
    torch::Tensor absgrad;
    auto t = BackwardImpl(&dL_dout_depth, &dL_dout_alpha, background, means3D, radii, colors, scales, rotations,
                          scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh,
                          degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug, &absgrad);
    return std::tuple_cat(std::move(t), std::make_tuple(absgrad));
}

// rasterize_gaussians_backward_absgrad's arguments, then the forward's opacities, its `antialiasing` and `absgrad`
// (false: the ninth tensor of the tuple comes back empty): gs4d_backward_aa, one entry for every combination
AbsgradTuple
RasterizeGaussiansBackwardAA(const torch::Tensor &background, const torch::Tensor &means3D, const torch::Tensor &radii,
                             const torch::Tensor &colors, const torch::Tensor &scales, const torch::Tensor &rotations,
                             const float scale_modifier, const torch::Tensor &cov3D_precomp,
                             const torch::Tensor &viewmatrix, const torch::Tensor &projmatrix, const float tan_fovx,
                             const float tan_fovy, const torch::Tensor &dL_dout_color,
                             const torch::Tensor &dL_dout_depth, const torch::Tensor &dL_dout_alpha,
                             const torch::Tensor &sh, const int degree, const torch::Tensor &campos,
                             const torch::Tensor &geomBuffer, const int R, const torch::Tensor &binningBuffer,
                             const torch::Tensor &imageBuffer, const bool debug, const torch::Tensor &opacities,
                             const bool antialiasing, const bool absgrad) {
    torch::Tensor abs = torch::empty({0}, means3D.options().dtype(torch::kFloat32));
    auto t = BackwardImpl(&dL_dout_depth, &dL_dout_alpha, background, means3D, radii, colors, scales, rotations,
                          scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh,
                          degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug, absgrad ? &abs : nullptr,
                          &opacities, antialiasing);
    return std::tuple_cat(std::move(t), std::make_tuple(abs));
}

// rasterize_gaussians_backward_aa's arguments; returns its tuple plus dL_dviewmatrix (4, 4), dL_dprojmatrix (4, 4) and
// dL_dcampos (3), indexed as the matrices the caller passed are (whatever their strides): gs4d_backward_camera
using CameraTuple = std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
                               torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>;
CameraTuple
RasterizeGaussiansBackwardCamera(const torch::Tensor &background, const torch::Tensor &means3D,
                                 const torch::Tensor &radii, const torch::Tensor &colors, const torch::Tensor &scales,
                                 const torch::Tensor &rotations, const float scale_modifier,
                                 const torch::Tensor &cov3D_precomp, const torch::Tensor &viewmatrix,
                                 const torch::Tensor &projmatrix, const float tan_fovx, const float tan_fovy,
                                 const torch::Tensor &dL_dout_color, const torch::Tensor &dL_dout_depth,
                                 const torch::Tensor &dL_dout_alpha, const torch::Tensor &sh, const int degree,
                                 const torch::Tensor &campos, const torch::Tensor &geomBuffer, const int R,
                                 const torch::Tensor &binningBuffer, const torch::Tensor &imageBuffer, const bool debug,
                                 const torch::Tensor &opacities, const bool antialiasing, const bool absgrad) {
    torch::Tensor abs = torch::empty({0}, means3D.options().dtype(torch::kFloat32));
    torch::Tensor cam;
    auto t = BackwardImpl(&dL_dout_depth, &dL_dout_alpha, background, means3D, radii, colors, scales, rotations,
                          scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh,
                          degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug, absgrad ? &abs : nullptr,
                          &opacities, antialiasing, &cam);
    return std::tuple_cat(std::move(t), std::make_tuple(abs, cam.slice(0, 0, 16).view({4, 4}),
                                                        cam.slice(0, 16, 32).view({4, 4}), cam.slice(0, 32, 35)));
}

// conic_opacity.w of the forward that filled geomBuffer, (P,): gs4d_debug_effective_opacity
torch::Tensor DebugEffectiveOpacity(const torch::Tensor &geomBuffer, const int P) {
    TORCH_CHECK(geomBuffer.is_cuda() && geomBuffer.scalar_type() == torch::kByte && P >= 0,
                "debug_effective_opacity: the geometry state of a forward over P Gaussians");
    const c10::hip::HIPGuard guard(geomBuffer.device().index());
    torch::Tensor out = torch::empty({P}, geomBuffer.options().dtype(torch::kFloat32));
    if (P == 0) return out;
    TORCH_CHECK(geomBuffer.numel() >= 64LL * P, "debug_effective_opacity: geomBuffer is too small for P Gaussians");
    check_status(gs4d_debug_effective_opacity(P, reinterpret_cast<const char *>(geomBuffer.data_ptr()),
                                              out.data_ptr<float>(),
                                              (void *)c10::hip::getCurrentHIPStream(geomBuffer.device().index()).stream()),
                 "debug_effective_opacity");
    return out;
}

// the per-tile instance lists of the forward that filled the three buffers, in render order: gs4d_debug_tile_lists.
// Returns (ranges (T, 2), order (T,), L', gid (L',), reach (L',), slot (L',), depth (L',)): int32 but the fp32 depth
std::tuple<torch::Tensor, torch::Tensor, int, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
DebugTileLists(const torch::Tensor &geomBuffer, const torch::Tensor &binningBuffer, const torch::Tensor &imgBuffer,
               const int P, const int W, const int H, const int num_rendered) {
    TORCH_CHECK(geomBuffer.is_cuda() && imgBuffer.is_cuda() && geomBuffer.scalar_type() == torch::kByte &&
                    imgBuffer.scalar_type() == torch::kByte && binningBuffer.scalar_type() == torch::kByte &&
                    P > 0 && W > 0 && H > 0 && num_rendered >= 0,
                "debug_tile_lists: the three states of a forward over P > 0 Gaussians and a W x H image");
    TORCH_CHECK(num_rendered == 0 || (binningBuffer.is_cuda() && binningBuffer.device() == geomBuffer.device()),
                "debug_tile_lists: binningBuffer must be on the geometry state's device");
    TORCH_CHECK(imgBuffer.device() == geomBuffer.device(), "debug_tile_lists: buffers on different devices");
    const long long T = (long long)((W + 15) / 16) * ((H + 15) / 16);
    TORCH_CHECK(geomBuffer.numel() >= 64LL * P, "debug_tile_lists: geomBuffer is too small for P Gaussians");
    TORCH_CHECK(imgBuffer.numel() >= 8LL * W * H + 12 * T, "debug_tile_lists: imgBuffer is not a W x H image state");
    TORCH_CHECK(binningBuffer.numel() >= 20LL * num_rendered,
                "debug_tile_lists: binningBuffer is too small for num_rendered instances");
    const c10::hip::HIPGuard guard(geomBuffer.device().index());
    const auto iopts = geomBuffer.options().dtype(torch::kInt32);
    torch::Tensor ranges = torch::empty({T, 2}, iopts), order = torch::empty({T}, iopts);
    torch::Tensor n = torch::empty({1}, iopts);
    torch::Tensor gid = torch::empty({num_rendered}, iopts), reach = torch::empty({num_rendered}, iopts),
                  slot = torch::empty({num_rendered}, iopts);
    torch::Tensor depth = torch::empty({num_rendered}, geomBuffer.options().dtype(torch::kFloat32));
    const auto u32 = [](torch::Tensor &t) { return t.numel() ? reinterpret_cast<uint32_t *>(t.data_ptr<int>()) : nullptr; };
    check_status(gs4d_debug_tile_lists(P, W, H, num_rendered, reinterpret_cast<const char *>(geomBuffer.data_ptr()),
                                       num_rendered ? reinterpret_cast<const char *>(binningBuffer.data_ptr()) : nullptr,
                                       reinterpret_cast<const char *>(imgBuffer.data_ptr()), u32(ranges), u32(order),
                                       u32(n), u32(gid), u32(reach), u32(slot),
                                       depth.numel() ? depth.data_ptr<float>() : nullptr,
                                       (void *)c10::hip::getCurrentHIPStream(geomBuffer.device().index()).stream()),
                 "debug_tile_lists");
    const int L = std::min(std::max(n.item<int>(), 0), num_rendered);
    return std::make_tuple(ranges, order, L, gid.slice(0, 0, L), reach.slice(0, 0, L), slot.slice(0, 0, L),
                           depth.slice(0, 0, L));
}

// the alpha image 1 - T_final (1, H, W) of the forward that filled imageBuffer: gs4d_alpha_image
torch::Tensor AlphaImage(const torch::Tensor &imageBuffer, const int image_height, const int image_width) {
    if (!imageBuffer.is_cuda())
        throw std::runtime_error("imageBuffer must be a HIP (GPU) tensor; the MI355X rasterizer has no CPU path");
    if (image_height <= 0 || image_width <= 0) throw std::runtime_error("alpha_image: the image must be non-empty");
    const long long need = 8LL * image_height * image_width;  // final_T and n_contrib precede the tile tables
    if (imageBuffer.scalar_type() != torch::kByte || imageBuffer.numel() < need)
        throw std::runtime_error("alpha_image: imageBuffer is not the image state of an H x W forward");
    const auto dev = imageBuffer.device();
    c10::hip::HIPGuard guard(dev.index());
    torch::Tensor out = torch::empty({1, image_height, image_width}, imageBuffer.options().dtype(torch::kFloat32));
    hipStream_t stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
    check_status(gs4d_alpha_image(image_width, image_height, reinterpret_cast<const char *>(imageBuffer.data_ptr()),
                                  out.data_ptr<float>(), (void *)stream),
                 "alpha_image");
    return out;
}

// rasterize_points.cu:200-219
torch::Tensor MarkVisible(torch::Tensor &means3D, torch::Tensor &viewmatrix, torch::Tensor &projmatrix) {
    const int P = means3D.size(0);
    torch::Tensor present = torch::full({P}, false, means3D.options().dtype(at::kBool));
    if (P != 0) {
        if (!means3D.is_cuda()) throw std::runtime_error("means3D must be a HIP (GPU) tensor; the MI355X rasterizer has no CPU path");
        const auto dev = means3D.device();
        c10::hip::HIPGuard guard(dev.index());
        auto m3 = prep(means3D, "means3D", dev), pm = prep(projmatrix, "projmatrix", dev);
        int vt = 0;
        auto vm = prep_view(viewmatrix, dev, vt);
        hipStream_t stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
        int st = gs4d_mark_visible_ex(P, fptr(m3), fptr(vm), fptr(pm),
                                      reinterpret_cast<uint8_t *>(present.data_ptr<bool>()), (void *)stream, vt);
        check_status(st, "mark_visible");
    }
    return present;
}

static std::vector<std::tuple<std::string, float>> last_timings() {
    const char *names[64];
    float ms[64];
    int n = gs4d_last_timings(names, ms, 64);
    std::vector<std::tuple<std::string, float>> out;
    for (int i = 0; i < n && i < 64; i++) out.emplace_back(names[i], ms[i]);
    return out;
}

// ext.cpp:15-18 plus three introspection helpers used by bench.py
// parity-test diagnostic: (o G, log2 G) of (Gaussian, pixel) pairs by the blend kernels' arithmetic
std::tuple<torch::Tensor, torch::Tensor> DebugPairAlpha(const torch::Tensor &geomBuffer, int P, int W, int H,
                                                        const torch::Tensor &gid_, const torch::Tensor &px_,
                                                        const torch::Tensor &py_) {
    TORCH_CHECK(geomBuffer.is_cuda() && gid_.is_cuda(), "debug_pair_alpha: device tensors");
    const c10::hip::HIPGuard guard(geomBuffer.device().index());
    auto gid = gid_.to(torch::kInt32).contiguous(), px = px_.to(torch::kInt32).contiguous(),
         py = py_.to(torch::kInt32).contiguous();
    TORCH_CHECK(gid.numel() == px.numel() && gid.numel() == py.numel(), "debug_pair_alpha: pair arrays differ");
    TORCH_CHECK(gid.numel() == 0 || (gid.min().item<int>() >= 0 && gid.max().item<int>() < P &&
                                     px.min().item<int>() >= 0 && py.min().item<int>() >= 0),
                "debug_pair_alpha: pair out of range");
    auto og = torch::empty({gid.numel()}, geomBuffer.options().dtype(torch::kFloat32));
    auto pw = torch::empty_like(og);
    const int st = gs4d_debug_pair_alpha(P, W, H, (const char *)geomBuffer.data_ptr(), (int)gid.numel(),
                                         gid.data_ptr<int>(), px.data_ptr<int>(), py.data_ptr<int>(),
                                         og.data_ptr<float>(), pw.data_ptr<float>(),
                                         c10::hip::getCurrentHIPStream(geomBuffer.device().index()).stream());
    TORCH_CHECK(st == 0, "debug_pair_alpha: ", gs4d_last_error());
    return {og, pw};
}

// reduction diagnostic: inputs n x 20 x 64 fp32 -> the n x 24 records by LDS column sums and by permlane swaps
std::tuple<torch::Tensor, torch::Tensor> DebugWaveSum(const torch::Tensor &in_, bool depth, bool abs) {
    TORCH_CHECK(in_.is_cuda() && in_.dim() == 3 && in_.size(1) == 20 && in_.size(2) == 64,
                "debug_wave_sum: a device tensor n x 20 x 64");
    const c10::hip::HIPGuard guard(in_.device().index());
    auto in = in_.to(torch::kFloat32).contiguous();
    const int n = (int)in.size(0);
    auto out_lds = torch::empty({n, 24}, in.options());
    auto out_permlane = torch::empty({n, 24}, in.options());
    const int st = gs4d_debug_wave_sum(n, in.data_ptr<float>(), depth, abs, out_lds.data_ptr<float>(),
                                       out_permlane.data_ptr<float>(),
                                       c10::hip::getCurrentHIPStream(in.device().index()).stream());
    TORCH_CHECK(st == 0, "debug_wave_sum: ", gs4d_last_error());
    return {out_lds, out_permlane};
}
static int DebugBackwardOccupancy(bool depth, bool abs) {
    int wgs = 0;
    TORCH_CHECK(gs4d_debug_backward_occupancy(depth, abs, &wgs) == 0, "debug_backward_occupancy: ", gs4d_last_error());
    return wgs;
}

// importance_glue.cpp, compiled into this module: the opt-in blend-weight importance binding
void bind_importance(pybind11::module_ &m);
void bind_features(pybind11::module_ &m);

PYBIND11_MODULE(_C, m) {
    m.def("rasterize_gaussians", &RasterizeGaussians);
    m.def("debug_pair_alpha", &DebugPairAlpha);
    m.def("debug_wave_sum", &DebugWaveSum);
    m.def("debug_backward_occupancy", &DebugBackwardOccupancy);
    m.def("rasterize_gaussians_backward", &RasterizeGaussiansBackward);
    m.def("rasterize_gaussians_backward_depth", &RasterizeGaussiansBackwardDepth);
    m.def("rasterize_gaussians_backward_aux", &RasterizeGaussiansBackwardAux);
    m.def("rasterize_gaussians_backward_absgrad", &RasterizeGaussiansBackwardAbsgrad);
    m.def("rasterize_gaussians_aa", &RasterizeGaussiansAA);
    m.def("rasterize_gaussians_backward_aa", &RasterizeGaussiansBackwardAA);
    m.def("rasterize_gaussians_backward_camera", &RasterizeGaussiansBackwardCamera);
    m.def("debug_effective_opacity", &DebugEffectiveOpacity);
    m.def("debug_tile_lists", &DebugTileLists);
    m.def("alpha_image", &AlphaImage);
    bind_importance(m);  // importance_glue.cpp: gaussian_importance
    bind_features(m);    // features_glue.cpp: rasterize_features, rasterize_features_backward, FEATURE_CHUNK
    m.def("mark_visible", &MarkVisible);
    m.def("set_profiling", [](int level) { gs4d_set_profiling(level); });
    m.def("last_timings", &last_timings);
    m.def("version", []() { return std::string(gs4d_version()); });
}
