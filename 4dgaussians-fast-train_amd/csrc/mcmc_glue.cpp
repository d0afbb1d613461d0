// mcmc_glue.cpp -- the train step's `_C` binding of the opt-in MCMC densification kernels (csrc/mcmc.hip; no
// counterpart in the reference): the counter-based generator's words, the opacity-proportional sampler, the
// correction of the sampled sources, the per-step position noise, the opacity / scale regulariser and the zeroing of
// moment rows.  Compiled into the same extension module as train_glue.cpp, whose PYBIND11_MODULE calls bind_mcmc.
// Every entry runs on its tensors' device and the current stream of that device.
#include <ATen/ATen.h>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include <string>
#include <tuple>
#include <vector>

#include "../../include/gs4d.h"
#include "../../include/gs4d_train.h"

namespace {

// the scratch allocator callback: one fresh byte tensor per call, kept alive until the launches are queued
char *scratch_cb(void *ctx, size_t n) {
    auto *t = static_cast<torch::Tensor *>(ctx);
    *t = torch::empty({(long long)n}, t->options());
    return reinterpret_cast<char *>(t->data_ptr());
}

void need(bool ok, const char *fn, const char *msg) {
    if (!ok) throw std::runtime_error(std::string(fn) + ": " + msg);
}

void check(int st, const char *fn) {
    if (st != GS4D_OK) throw std::runtime_error(std::string(fn) + ": " + gs4d_last_error());
}

bool gpu_f32(const torch::Tensor &t) { return t.is_cuda() && t.scalar_type() == torch::kFloat32 && t.is_contiguous(); }
bool gpu_i32(const torch::Tensor &t) { return t.is_cuda() && t.scalar_type() == torch::kInt32 && t.is_contiguous(); }

hipStream_t stream_of(const torch::Tensor &t) { return c10::hip::getCurrentHIPStream(t.device().index()).stream(); }

uint32_t word(int64_t v, const char *fn, const char *what) {
    need(v >= 0 && v <= 0xffffffffll, fn, what);
    return (uint32_t)v;
}

}  // namespace

// the four words of Philox blocks 0 .. n - 1 written into out (n, 4) int32 (the words' bits); returns out
static torch::Tensor mcmc_random_bits(torch::Tensor out, uint64_t seed, int64_t iteration, int64_t purpose) {
    const char *fn = "mcmc_random_bits";
    need(gpu_i32(out) && out.dim() == 2 && out.size(1) == 4, fn, "out must be a contiguous (n, 4) int32 HIP (GPU) tensor");
    need(out.size(0) <= 0x7fffffffll, fn, "at most 2^31 - 1 blocks");
    c10::hip::HIPGuard guard(out.device().index());
    check(gs4d_mcmc_random_bits((int)out.size(0), seed, word(iteration, fn, "iteration must fit 32 bits"),
                                word(purpose, fn, "purpose must fit 32 bits"), (uint32_t *)out.data_ptr<int32_t>(),
                                (void *)stream_of(out)),
          fn);
    return out;
}

// (draws (n) int32, counts (P) int32, n_drawn (1) int32) of n opacity-proportional draws; opacity: the ACTIVATED
// opacities, (P) or (P, 1)
static std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> mcmc_sample(const torch::Tensor &opacity, double min_opacity,
                                                                           int64_t n, uint64_t seed, int64_t iteration,
                                                                           int64_t purpose) {
    const char *fn = "mcmc_sample";
    need(gpu_f32(opacity) && (opacity.dim() == 1 || (opacity.dim() == 2 && opacity.size(1) == 1)), fn,
         "opacity must be a contiguous (P) or (P, 1) float32 HIP (GPU) tensor");
    const int64_t P = opacity.size(0);
    need(P <= 0x7fffffffll && n >= 0 && n <= 0x7fffffffll, fn, "P and n must be in 0 .. 2^31 - 1");
    need(min_opacity >= 0.0, fn, "min_opacity must be >= 0");
    c10::hip::HIPGuard guard(opacity.device().index());
    const auto iopt = opacity.options().dtype(torch::kInt32);
    torch::Tensor draws = torch::zeros({n}, iopt), counts = torch::zeros({P}, iopt), n_drawn = torch::zeros({1}, iopt);
    torch::Tensor scratch = torch::empty({0}, opacity.options().dtype(torch::kByte));
    check(gs4d_mcmc_sample((int)P, opacity.data_ptr<float>(), (float)min_opacity, (int)n, seed,
                           word(iteration, fn, "iteration must fit 32 bits"), word(purpose, fn, "purpose must fit 32 bits"),
                           draws.data_ptr<int32_t>(), counts.data_ptr<int32_t>(), n_drawn.data_ptr<int32_t>(), scratch_cb,
                           &scratch, (void *)stream_of(opacity)),
          fn);
    return std::make_tuple(draws, counts, n_drawn);
}

// in place on the raw opacity (P, 1) and scaling (P, 3): the correction of the rows with counts > 0
static void mcmc_relocate(torch::Tensor opacity_raw, torch::Tensor scaling_raw, const torch::Tensor &counts,
                          double min_opacity) {
    const char *fn = "mcmc_relocate";
    need(gpu_f32(opacity_raw) && opacity_raw.dim() <= 2, fn, "opacity must be a contiguous (P, 1) float32 HIP (GPU) tensor");
    const int64_t P = opacity_raw.numel();
    need(gpu_f32(scaling_raw) && scaling_raw.dim() == 2 && scaling_raw.size(0) == P && scaling_raw.size(1) == 3 &&
             scaling_raw.device() == opacity_raw.device(),
         fn, "scaling must be a contiguous (P, 3) float32 tensor on opacity's device");
    need(gpu_i32(counts) && counts.numel() == P && counts.device() == opacity_raw.device(), fn,
         "counts must be a contiguous (P) int32 tensor on opacity's device");
    need(P <= 0x7fffffffll, fn, "P must be below 2^31");
    c10::hip::HIPGuard guard(opacity_raw.device().index());
    check(gs4d_mcmc_relocate((int)P, counts.data_ptr<int32_t>(), (float)min_opacity, opacity_raw.data_ptr<float>(),
                             scaling_raw.data_ptr<float>(), (void *)stream_of(opacity_raw)),
          fn);
}

// in place on xyz (P, 3): the per-step noise; normals (P, 3) replaces the generated draws
static void mcmc_noise(torch::Tensor xyz, const torch::Tensor &scaling_raw, const torch::Tensor &rotation_raw,
                       const torch::Tensor &opacity_raw, double step_scale, uint64_t seed, int64_t iteration,
                       const c10::optional<torch::Tensor> &normals) {
    const char *fn = "mcmc_noise";
    need(gpu_f32(xyz) && xyz.dim() == 2 && xyz.size(1) == 3, fn, "xyz must be a contiguous (P, 3) float32 HIP (GPU) tensor");
    const int64_t P = xyz.size(0);
    need(P <= 0x7fffffffll, fn, "P must be below 2^31");
    need(gpu_f32(scaling_raw) && scaling_raw.dim() == 2 && scaling_raw.size(0) == P && scaling_raw.size(1) == 3 &&
             scaling_raw.device() == xyz.device(),
         fn, "scaling must be a contiguous (P, 3) float32 tensor on xyz's device");
    need(gpu_f32(rotation_raw) && rotation_raw.dim() == 2 && rotation_raw.size(0) == P && rotation_raw.size(1) == 4 &&
             rotation_raw.device() == xyz.device(),
         fn, "rotation must be a contiguous (P, 4) float32 tensor on xyz's device");
    need(gpu_f32(opacity_raw) && opacity_raw.numel() == P && opacity_raw.device() == xyz.device(), fn,
         "opacity must be a contiguous (P, 1) float32 tensor on xyz's device");
    if (normals.has_value())
        need(gpu_f32(*normals) && normals->sizes() == xyz.sizes() && normals->device() == xyz.device(), fn,
             "normals must be a contiguous (P, 3) float32 tensor on xyz's device");
    c10::hip::HIPGuard guard(xyz.device().index());
    check(gs4d_mcmc_noise((int)P, xyz.data_ptr<float>(), scaling_raw.data_ptr<float>(), rotation_raw.data_ptr<float>(),
                          opacity_raw.data_ptr<float>(), (float)step_scale, seed,
                          word(iteration, fn, "iteration must fit 32 bits"),
                          normals.has_value() ? normals->data_ptr<float>() : nullptr, (void *)stream_of(xyz)),
          fn);
}

// the regulariser's value (0-dim); its gradient is added into grad_opacity / grad_scaling where given
static torch::Tensor mcmc_reg_grad(const torch::Tensor &opacity_raw, const torch::Tensor &scaling_raw, double w_opacity,
                                   double w_scale, c10::optional<torch::Tensor> grad_opacity,
                                   c10::optional<torch::Tensor> grad_scaling) {
    const char *fn = "mcmc_reg_grad";
    need(gpu_f32(opacity_raw) && opacity_raw.dim() <= 2, fn, "opacity must be a contiguous (P, 1) float32 HIP (GPU) tensor");
    const int64_t P = opacity_raw.numel();
    need(P <= 0x7fffffffll, fn, "P must be below 2^31");
    need(gpu_f32(scaling_raw) && scaling_raw.dim() == 2 && scaling_raw.size(0) == P && scaling_raw.size(1) == 3 &&
             scaling_raw.device() == opacity_raw.device(),
         fn, "scaling must be a contiguous (P, 3) float32 tensor on opacity's device");
    if (grad_opacity.has_value())
        need(gpu_f32(*grad_opacity) && grad_opacity->numel() == P && grad_opacity->device() == opacity_raw.device(), fn,
             "grad_opacity must be a contiguous float32 tensor of opacity's size and device");
    if (grad_scaling.has_value())
        need(gpu_f32(*grad_scaling) && grad_scaling->sizes() == scaling_raw.sizes() &&
                 grad_scaling->device() == opacity_raw.device(),
             fn, "grad_scaling must be a contiguous float32 tensor of scaling's size and device");
    c10::hip::HIPGuard guard(opacity_raw.device().index());
    torch::Tensor value = torch::zeros({}, opacity_raw.options());
    torch::Tensor scratch = torch::empty({0}, opacity_raw.options().dtype(torch::kByte));
    check(gs4d_mcmc_reg_grad((int)P, opacity_raw.data_ptr<float>(), scaling_raw.data_ptr<float>(), (float)w_opacity,
                             (float)w_scale, value.data_ptr<float>(),
                             grad_opacity.has_value() ? grad_opacity->data_ptr<float>() : nullptr,
                             grad_scaling.has_value() ? grad_scaling->data_ptr<float>() : nullptr, scratch_cb, &scratch,
                             (void *)stream_of(opacity_raw)),
          fn);
    return value;
}

// rows `rows` (int32) of every tensor (P, ...) set to zero, in place, one launch for all of them
static void mcmc_zero_rows(std::vector<torch::Tensor> tensors, const torch::Tensor &rows) {
    const char *fn = "mcmc_zero_rows";
    need(gpu_i32(rows) && rows.dim() == 1, fn, "rows must be a contiguous int32 HIP (GPU) vector");
    need((int64_t)tensors.size() <= GS4D_ROWS_MAX_TENSORS, fn, "at most 32 tensors");
    if (tensors.empty()) return;
    gs4d_zero_rows_batch b;
    b.count = (int)tensors.size();
    b.P = tensors[0].dim() >= 1 ? tensors[0].size(0) : -1;
    b.n = rows.numel();
    b.rows = rows.data_ptr<int32_t>();
    for (int i = 0; i < b.count; i++) {
        const torch::Tensor &t = tensors[i];
        need(gpu_f32(t) && t.dim() >= 1 && t.size(0) == b.P && t.device() == rows.device(), fn,
             "tensors must be contiguous float32 tensors of one row count on the rows' device");
        b.t[i].data = t.data_ptr<float>();
        b.t[i].width = b.P > 0 ? t.numel() / b.P : 1;
    }
    c10::hip::HIPGuard guard(rows.device().index());
    check(gs4d_mcmc_zero_rows(&b, (void *)stream_of(rows)), fn);
}

void bind_mcmc(pybind11::module_ &m) {
    namespace py = pybind11;
    m.def("mcmc_random_bits", &mcmc_random_bits, py::arg("out"), py::arg("seed"), py::arg("iteration"), py::arg("purpose"));
    m.def("mcmc_sample", &mcmc_sample, py::arg("opacity"), py::arg("min_opacity"), py::arg("n"), py::arg("seed"),
          py::arg("iteration"), py::arg("purpose"));
    m.def("mcmc_relocate", &mcmc_relocate, py::arg("opacity"), py::arg("scaling"), py::arg("counts"),
          py::arg("min_opacity"));
    m.def("mcmc_noise", &mcmc_noise, py::arg("xyz"), py::arg("scaling"), py::arg("rotation"), py::arg("opacity"),
          py::arg("step_scale"), py::arg("seed"), py::arg("iteration"), py::arg("normals") = py::none());
    m.def("mcmc_reg_grad", &mcmc_reg_grad, py::arg("opacity"), py::arg("scaling"), py::arg("w_opacity"), py::arg("w_scale"),
          py::arg("grad_opacity"), py::arg("grad_scaling"));
    m.def("mcmc_zero_rows", &mcmc_zero_rows, py::arg("tensors"), py::arg("rows"));
}
