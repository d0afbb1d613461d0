// importance_glue.cpp -- the `_C` module's binding of gs4d_importance, the opt-in per-Gaussian blend-weight scores
// (no counterpart in the reference's rasterize_points.cu / ext.cpp, which torch_glue.cpp mirrors).  Compiled into the
// same extension module as torch_glue.cpp, whose PYBIND11_MODULE calls bind_importance.
#include <ATen/ATen.h>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include <string>
#include <tuple>

#include "../../include/gs4d.h"

namespace {

// the scratch allocator callback: one fresh byte tensor per call, kept alive until the launches are queued (the
// caching allocator keeps the block for the stream it was allocated on)
char *scratch_cb(void *ctx, size_t n) {
    auto *t = static_cast<torch::Tensor *>(ctx);
    *t = torch::empty({(long long)n}, t->options());
    return reinterpret_cast<char *>(t->data_ptr());
}

}  // namespace

// the per-Gaussian blend-weight scores (weight_sum, weight_max, pixel_count) of the forward that filled the three
// buffers: gs4d_importance, on the current stream of the buffers' device
static std::tuple<torch::Tensor, torch::Tensor, torch::Tensor>
GaussianImportance(const torch::Tensor &geomBuffer, const torch::Tensor &binningBuffer, const torch::Tensor &imageBuffer,
                   const int num_rendered, const int P, const int image_height, const int image_width) {
    if (!geomBuffer.is_cuda() || !imageBuffer.is_cuda() || (num_rendered > 0 && !binningBuffer.is_cuda()))
        throw std::runtime_error("gaussian_importance: the buffers must be HIP (GPU) tensors; the MI355X rasterizer has no CPU path");
    if (P < 0) throw std::runtime_error("gaussian_importance: P must be >= 0");
    const auto dev = geomBuffer.device();
    c10::hip::HIPGuard guard(dev.index());
    auto float_opts = geomBuffer.options().dtype(torch::kFloat32);
    torch::Tensor wsum = torch::empty({P}, float_opts), wmax = torch::empty({P}, float_opts);
    torch::Tensor count = torch::empty({P}, geomBuffer.options().dtype(torch::kInt32));
    torch::Tensor scratch = torch::empty({0}, geomBuffer.options().dtype(torch::kByte));
    hipStream_t stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
    const int st = gs4d_importance(
        P, image_width, image_height, num_rendered, reinterpret_cast<const char *>(geomBuffer.data_ptr()),
        num_rendered > 0 ? reinterpret_cast<const char *>(binningBuffer.data_ptr()) : nullptr,
        reinterpret_cast<const char *>(imageBuffer.data_ptr()), P ? wsum.data_ptr<float>() : nullptr,
        P ? wmax.data_ptr<float>() : nullptr, P ? count.data_ptr<int32_t>() : nullptr, scratch_cb, &scratch,
        (void *)stream);
    if (st != GS4D_OK) throw std::runtime_error(std::string("gaussian_importance: ") + gs4d_last_error());
    return std::make_tuple(wsum, wmax, count);
}

void bind_importance(pybind11::module_ &m) { m.def("gaussian_importance", &GaussianImportance); }
