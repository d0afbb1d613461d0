// rigidity_glue.cpp -- the train step's `_C` binding of gs4d_isometry_loss_grad, the opt-in local-isometry
// regulariser over a K-NN graph (csrc/rigidity.hip; no counterpart in the reference).  Compiled into the same
// extension module as train_glue.cpp, whose PYBIND11_MODULE calls bind_rigidity.
#include <ATen/ATen.h>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include <string>
#include <tuple>

#include "../../include/gs4d.h"
#include "../../include/gs4d_train.h"

namespace {

// the scratch allocator callback: one fresh byte tensor per call, kept alive until the launches are queued
char *scratch_cb(void *ctx, size_t n) {
    auto *t = static_cast<torch::Tensor *>(ctx);
    *t = torch::empty({(long long)n}, t->options());
    return reinterpret_cast<char *>(t->data_ptr());
}

void need(bool ok, const char *msg) {
    if (!ok) throw std::runtime_error(std::string("isometry_loss_grad: ") + msg);
}

}  // namespace

// (value (0-dim), dL/dxa or None, dL/dxb or None) of scale / E * sum_e w_e (r_b - r_a)^2 over the graph's valid
// edges, on the positions' device and the current stream; weights = None stands for ones
static std::tuple<torch::Tensor, c10::optional<torch::Tensor>, c10::optional<torch::Tensor>>
isometry_loss_grad(const torch::Tensor &nbr_idx, const torch::Tensor &in_start, const torch::Tensor &in_edge,
                   const c10::optional<torch::Tensor> &weights, const torch::Tensor &xa, const torch::Tensor &xb,
                   double scale, bool want_a, bool want_b) {
    need(xa.is_cuda() && xa.scalar_type() == torch::kFloat32 && xa.is_contiguous() && xa.dim() == 2 && xa.size(1) == 3,
         "xa must be a contiguous (P, 3) float32 HIP (GPU) tensor");
    need(xb.is_cuda() && xb.scalar_type() == torch::kFloat32 && xb.is_contiguous() && xb.sizes() == xa.sizes() &&
             xb.device() == xa.device(),
         "xb must match xa");
    const int64_t P = xa.size(0);
    need(nbr_idx.dim() == 2 && nbr_idx.size(0) == P, "nbr_idx must be (P, K)");
    const int64_t K = nbr_idx.size(1);
    need(K >= 1 && K <= 16, "K must be in 1..16");
    need(in_start.numel() == P + 1 && in_edge.numel() == P * K, "in_start must hold P + 1 and in_edge P K entries");
    for (const torch::Tensor *t : {&nbr_idx, &in_start, &in_edge})
        need(t->device() == xa.device() && t->scalar_type() == torch::kInt32 && t->is_contiguous(),
             "the graph must be contiguous int32 tensors on the positions' device");
    if (weights.has_value())
        need(weights->device() == xa.device() && weights->scalar_type() == torch::kFloat32 && weights->is_contiguous() &&
                 weights->numel() == P * K,
             "weights must be a contiguous (P, K) float32 tensor on the positions' device");
    c10::hip::HIPGuard guard(xa.device().index());
    torch::Tensor value = torch::zeros({}, xa.options());
    c10::optional<torch::Tensor> ga, gb;
    if (want_a) ga = torch::empty_like(xa);
    if (want_b) gb = torch::empty_like(xb);
    if (P == 0) return std::make_tuple(value, ga, gb);
    torch::Tensor scratch = torch::empty({0}, xa.options().dtype(torch::kByte));
    hipStream_t stream = c10::hip::getCurrentHIPStream(xa.device().index()).stream();
    const int st = gs4d_isometry_loss_grad(
        (int)P, (int)K, nbr_idx.data_ptr<int32_t>(), in_start.data_ptr<int32_t>(), in_edge.data_ptr<int32_t>(),
        weights.has_value() ? weights->data_ptr<float>() : nullptr, xa.data_ptr<float>(), xb.data_ptr<float>(),
        (float)scale, value.data_ptr<float>(), want_a ? ga->data_ptr<float>() : nullptr,
        want_b ? gb->data_ptr<float>() : nullptr, scratch_cb, &scratch, (void *)stream);
    if (st != GS4D_OK) throw std::runtime_error(std::string("isometry_loss_grad: ") + gs4d_last_error());
    return std::make_tuple(value, ga, gb);
}

void bind_rigidity(pybind11::module_ &m) {
    m.def("isometry_loss_grad", &isometry_loss_grad, pybind11::arg("nbr_idx"), pybind11::arg("in_start"),
          pybind11::arg("in_edge"), pybind11::arg("weights"), pybind11::arg("xa"), pybind11::arg("xb"),
          pybind11::arg("scale"), pybind11::arg("want_a"), pybind11::arg("want_b"));
}
