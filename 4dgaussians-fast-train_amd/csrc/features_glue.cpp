// features_glue.cpp -- the `_C` module's binding of gs4d_features_forward / gs4d_features_backward, the opt-in
// N-channel feature rendering (no counterpart in the reference's rasterize_points.cu / ext.cpp, which torch_glue.cpp
// mirrors).  Compiled into the same extension module as torch_glue.cpp, whose PYBIND11_MODULE calls bind_features.
#include <ATen/ATen.h>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include <string>
#include <tuple>

#include "../../include/gs4d.h"

namespace {

// the scratch allocator callback: one fresh byte tensor per call, kept alive until the launches are queued
char *scratch_cb(void *ctx, size_t n) {
    auto *t = static_cast<torch::Tensor *>(ctx);
    *t = torch::empty({(long long)n}, t->options());
    return reinterpret_cast<char *>(t->data_ptr());
}

// a float32 tensor on `dev`, contiguous and 16-byte aligned (an empty tensor stays empty: "not provided")
torch::Tensor prep(const torch::Tensor &t, const char *name, const torch::Device &dev) {
    if (t.numel() == 0) return t;
    if (!t.is_cuda() || t.device() != dev)
        throw std::runtime_error(std::string("rasterize_features: ") + name + " must be a HIP (GPU) tensor on the buffers' device");
    if (t.scalar_type() != torch::kFloat32) throw std::runtime_error(std::string("rasterize_features: ") + name + " must be float32");
    torch::Tensor c = t.contiguous();
    if ((reinterpret_cast<uintptr_t>(c.data_ptr()) & 15) != 0) c = c.clone();
    return c;
}
const float *fptr(const torch::Tensor &t) { return t.numel() ? t.data_ptr<float>() : nullptr; }

void check_features(const torch::Tensor &features, int P) {
    if (features.dim() != 2 || features.size(0) != P || features.size(1) < 1)
        throw std::runtime_error("rasterize_features: features must have dimensions (num_points, C) with C >= 1");
}

// the forward's three state buffers live on the features' device (binning: only when an emission ran)
void check_buffers(const torch::Tensor &geom, const torch::Tensor &binning, const torch::Tensor &image, int num_rendered,
                   const torch::Device &dev) {
    if (!geom.is_cuda() || !image.is_cuda() || (num_rendered > 0 && !binning.is_cuda()))
        throw std::runtime_error("rasterize_features: the buffers must be HIP (GPU) tensors");
    if (geom.device() != dev || image.device() != dev || (num_rendered > 0 && binning.device() != dev))
        throw std::runtime_error("rasterize_features: the buffers must be on the features' device");
}

// the image state of a W x H forward: final_T, n_contrib and the tiles' ranges, each padded to 256 bytes, then the
// tiles' order and 512 bytes (capi.hip, ImageState::required, which sized the buffer rasterize_gaussians returned);
// another size means the (H, W) given here are not that forward's, and the state would be carved at wrong offsets
void check_image_size(const torch::Tensor &image, long long H, long long W) {
    const auto pad = [](long long n) { return (n + 255) / 256 * 256; };
    const long long N = H * W, T = ((W + 15) / 16) * ((H + 15) / 16);
    if (H <= 0 || W <= 0 || image.numel() != pad(4 * N) * 2 + pad(8 * T) + 4 * T + 512)
        throw std::runtime_error("rasterize_features: the image buffer is not the state of an H x W forward");
}

}  // namespace

// the feature image (C, H, W) of the forward that filled the three buffers: gs4d_features_forward, on the current
// stream of the buffers' device
static torch::Tensor RasterizeFeatures(const torch::Tensor &features, const torch::Tensor &geomBuffer,
                                       const int num_rendered, const torch::Tensor &binningBuffer,
                                       const torch::Tensor &imageBuffer, const int P, const int image_height,
                                       const int image_width) {
    if (!features.is_cuda()) throw std::runtime_error("rasterize_features: features must be a HIP (GPU) tensor; the MI355X rasterizer has no CPU path");
    check_features(features, P);
    const auto dev = features.device();
    c10::hip::HIPGuard guard(dev.index());
    const int C = (int)features.size(1);
    auto opts = features.options().dtype(torch::kFloat32);
    if (P == 0) return torch::zeros({C, image_height, image_width}, opts);
    check_buffers(geomBuffer, binningBuffer, imageBuffer, num_rendered, dev);
    check_image_size(imageBuffer, image_height, image_width);
    auto f = prep(features, "features", dev);
    torch::Tensor out = torch::empty({C, image_height, image_width}, opts);
    hipStream_t stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
    const int st = gs4d_features_forward(
        P, C, image_width, image_height, num_rendered, reinterpret_cast<const char *>(geomBuffer.data_ptr()),
        num_rendered > 0 ? reinterpret_cast<const char *>(binningBuffer.data_ptr()) : nullptr,
        reinterpret_cast<const char *>(imageBuffer.data_ptr()), fptr(f), out.data_ptr<float>(), nullptr, nullptr,
        (void *)stream);
    if (st != GS4D_OK) throw std::runtime_error(std::string("rasterize_features: ") + gs4d_last_error());
    return out;
}

// (dL_dfeatures, dL_dmeans2D, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dscales, dL_drotations) of the feature image:
// gs4d_features_backward.  geometry = false: only dL_dfeatures is computed and the six others are empty tensors.
// `opacities` and `antialiasing` as rasterize_gaussians_backward_aa takes them (an empty tensor and False for none).
static std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
RasterizeFeaturesBackward(const torch::Tensor &features, const torch::Tensor &dL_dout_features,
                          const torch::Tensor &means3D, const torch::Tensor &radii, const torch::Tensor &scales,
                          const torch::Tensor &rotations, const float scale_modifier, const torch::Tensor &cov3D_precomp,
                          const torch::Tensor &viewmatrix, const torch::Tensor &projmatrix, const float tan_fovx,
                          const float tan_fovy, const torch::Tensor &geomBuffer, const int R,
                          const torch::Tensor &binningBuffer, const torch::Tensor &imageBuffer,
                          const torch::Tensor &opacities, const bool antialiasing, const bool geometry) {
    if (!features.is_cuda()) throw std::runtime_error("rasterize_features_backward: features must be a HIP (GPU) tensor; the MI355X rasterizer has no CPU path");
    if (means3D.dim() != 2 || means3D.size(1) != 3)
        throw std::runtime_error("rasterize_features_backward: means3D must have dimensions (num_points, 3)");
    const int P = (int)means3D.size(0);
    check_features(features, P);
    const auto dev = features.device();
    c10::hip::HIPGuard guard(dev.index());
    const int C = (int)features.size(1);
    if (dL_dout_features.dim() != 3 || dL_dout_features.size(0) != C)
        throw std::runtime_error("rasterize_features_backward: grad_out_features must have dimensions (C, H, W)");
    const int H = (int)dL_dout_features.size(1), W = (int)dL_dout_features.size(2);
    auto opts = features.options().dtype(torch::kFloat32);
    const long long Pg = geometry ? P : 0;
    torch::Tensor dL_dfeatures = torch::empty({P, C}, opts);
    torch::Tensor dL_dmeans2D = torch::empty({Pg, 3}, opts), dL_dopacity = torch::empty({Pg, 1}, opts),
                  dL_dmeans3D = torch::empty({Pg, 3}, opts), dL_dcov3D = torch::empty({Pg, 6}, opts),
                  dL_dscales = torch::empty({Pg, 3}, opts), dL_drotations = torch::empty({Pg, 4}, opts);
    if (P != 0) {
        check_buffers(geomBuffer, binningBuffer, imageBuffer, R, dev);
        check_image_size(imageBuffer, H, W);  // (H, W) of the upstream image must be the forward's
        auto f = prep(features, "features", dev), dl = prep(dL_dout_features, "grad_out_features", dev),
             m3 = prep(means3D, "means3D", dev), sc = prep(scales, "scales", dev), rot = prep(rotations, "rotations", dev),
             c3 = prep(cov3D_precomp, "cov3D_precomp", dev), pm = prep(projmatrix, "projmatrix", dev),
             op = prep(opacities, "opacities", dev);
        // the view matrix as the reference's callers pass it (a transposed 4x4 view) is read in place
        int vt = 0;
        torch::Tensor vm = viewmatrix;
        if (vm.numel() == 16 && vm.dim() >= 2 && vm.size(-1) == 4 && vm.size(-2) == 4 && vm.stride(-1) == 4 &&
            vm.stride(-2) == 1 && vm.is_cuda() && vm.device() == dev && vm.scalar_type() == torch::kFloat32 &&
            (reinterpret_cast<uintptr_t>(vm.data_ptr()) & 15) == 0)
            vt = 1;
        else
            vm = prep(viewmatrix, "viewmatrix", dev);
        if (antialiasing && op.numel() != P) throw std::runtime_error("rasterize_features_backward: opacities must have P elements");
        torch::Tensor rad = radii.contiguous();
        if (rad.numel() && (rad.scalar_type() != torch::kInt32 || !rad.is_cuda()))
            throw std::runtime_error("rasterize_features_backward: radii must be an int32 GPU tensor");
        torch::Tensor scratch = torch::empty({0}, features.options().dtype(torch::kByte));
        hipStream_t stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
        const int st = gs4d_features_backward(
            P, C, R, W, H, fptr(m3), fptr(sc), scale_modifier, fptr(rot), fptr(c3), fptr(vm), fptr(pm), tan_fovx,
            tan_fovy, rad.numel() ? rad.data_ptr<int>() : nullptr, reinterpret_cast<char *>(geomBuffer.data_ptr()),
            binningBuffer.numel() ? reinterpret_cast<char *>(binningBuffer.data_ptr()) : nullptr,
            reinterpret_cast<char *>(imageBuffer.data_ptr()), fptr(f), fptr(dl), dL_dfeatures.data_ptr<float>(),
            geometry ? dL_dmeans2D.data_ptr<float>() : nullptr, geometry ? dL_dopacity.data_ptr<float>() : nullptr,
            geometry ? dL_dmeans3D.data_ptr<float>() : nullptr, geometry ? dL_dcov3D.data_ptr<float>() : nullptr,
            geometry ? dL_dscales.data_ptr<float>() : nullptr, geometry ? dL_drotations.data_ptr<float>() : nullptr,
            scratch_cb, &scratch, (void *)stream, vt, fptr(op), antialiasing ? 1 : 0);
        if (st != GS4D_OK) throw std::runtime_error(std::string("rasterize_features_backward: ") + gs4d_last_error());
    }
    return std::make_tuple(dL_dfeatures, dL_dmeans2D, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dscales, dL_drotations);
}

void bind_features(pybind11::module_ &m) {
    m.def("rasterize_features", &RasterizeFeatures);
    m.def("rasterize_features_backward", &RasterizeFeaturesBackward);
    m.attr("FEATURE_CHUNK") = gs4d_feature_chunk();
}
