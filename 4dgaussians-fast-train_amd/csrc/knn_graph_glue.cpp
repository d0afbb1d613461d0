// knn_graph_glue.cpp -- the `simple_knn._C` module's binding of gs4d_knn_graph, the opt-in exact K-NN graph with its
// transpose (no counterpart in the reference's simple-knn, which knn_glue.cpp mirrors).  Compiled into the same
// extension module as knn_glue.cpp, whose PYBIND11_MODULE calls bind_knn_graph.
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
}  // namespace

// knn_graph(points (P,3) float32, K in 1..16) -> (idx (P,K) int32, dist2 (P,K) float32, in_start (P+1,) int32,
// in_edge (P*K,) int32): gs4d_knn_graph on the points' device and the current stream (no reference counterpart)
// The input checks are distCUDA2's.
static std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor> knn_graph(const torch::Tensor &points, int K) {
    if (points.ndimension() != 2 || points.size(1) != 3) throw std::runtime_error("points must have dimensions (num_points, 3)");
    if (!points.is_cuda()) throw std::runtime_error("points must be a HIP (GPU) tensor; simple_knn has no CPU path");
    if (K < 1 || K > 16) throw std::runtime_error("knn_graph: K must be in 1..16");
    const int P = (int)points.size(0);
    c10::hip::HIPGuard guard(points.device().index());
    torch::Tensor pts = points.to(torch::kFloat32).contiguous();
    auto iopt = pts.options().dtype(torch::kInt32);
    torch::Tensor idx = torch::empty({P, K}, iopt), dist2 = torch::empty({P, K}, pts.options());
    torch::Tensor in_start = torch::zeros({P + 1}, iopt), in_edge = torch::empty({(long long)P * K}, iopt);
    if (P == 0) return std::make_tuple(idx, dist2, in_start, in_edge);
    torch::Tensor scratch = torch::empty({0}, pts.options().dtype(torch::kByte));
    hipStream_t stream = c10::hip::getCurrentHIPStream(points.device().index()).stream();
    int st = gs4d_knn_graph(P, K, pts.data_ptr<float>(), idx.data_ptr<int32_t>(), dist2.data_ptr<float>(),
                            in_start.data_ptr<int32_t>(), in_edge.data_ptr<int32_t>(), scratch_cb, &scratch, (void *)stream);
    if (st != GS4D_OK) throw std::runtime_error(std::string("knn_graph: ") + gs4d_last_error());
    return std::make_tuple(idx, dist2, in_start, in_edge);
}

void bind_knn_graph(pybind11::module_ &m) { m.def("knn_graph", &knn_graph, pybind11::arg("points"), pybind11::arg("K")); }
