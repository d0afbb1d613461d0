"""Scenes, a route restatement and reference runners for the tests of gs4d_train/deformation.py's dispatch
(tests/test_deformation_routes_boundary.py on the CPU, tests/test_deformation_routes_gpu.py on the GPU).

A scene is one row of SCENES: a small Deformation (one field for all: HexPlane resolution [8, 8, 8, 5], 16 or 32
features per level, as many levels as the wanted feat_dim needs), P points, a committed seed, the active heads and
the heads the loss reads.  The network and its inputs are drawn on the CPU from that seed (planes uniform in
[0.1, 0.5], Linears N(0, 1 / in), biases 0.1 N, points uniform in the bounds, upstream gradients N(0, 1)), so the
CPU preconditions and the GPU comparisons see the same numbers.

expected_calls restates the dispatch rule of Deformation._heads / _DeformHeads / _DeformHeadsBF16 / _splitk_dw from
their documentation: how often one forward plus backward calls each MLP entry of gs4d_train._C.  It does not import
gs4d_train.deformation."""
import collections
import copy

import numpy as np
import torch

HEADS = ("pos_deform", "scales_deform", "rotations_deform", "opacity_deform", "shs_deform")
HEAD_N = (3, 3, 4, 1, 48)
FLAGS = ("no_dx", "no_ds", "no_dr", "no_do", "no_dshs")
POS, SCALES, ROT, OPACITY, SHS = range(5)
THREE, FIVE = (POS, SCALES, ROT), (POS, SCALES, ROT, OPACITY, SHS)

Scene = collections.namedtuple("Scene", "name feat_dim W depth heads P seed loss dtype same_as")


def _s(name, feat_dim, W, depth, heads, P, seed, loss=None, dtype="fp32", same_as=None):
    return Scene(name, feat_dim, W, depth, tuple(heads), P, seed, tuple(loss if loss is not None else heads), dtype,
                 same_as)


# same_as: (scene, why) where a scene's call counts equal another's on purpose.  The seeds are those find_seed
# (below) returned; test_deformation_routes_boundary.py asserts what they guarantee.
SCENES = collections.OrderedDict((s.name, s) for s in (
    _s("dnerf", 64, 64, 0, THREE, 600, 9),
    _s("dynerf", 32, 128, 0, FIVE, 600, 3,
       same_as=("dnerf", "one launch per entry whatever the head set: the narrow group and the 48-wide head share them")),
    _s("w64_five", 64, 64, 0, FIVE, 600, 56, same_as=("dnerf", "the 48-wide head at W = 64 rides the same launches")),
    _s("default", 128, 64, 1, THREE, 2500, 2),
    _s("depth2", 32, 128, 2, THREE, 600, 15,
       same_as=("default", "_LinearSplitK is torch: one layer or two, split or not, no _C entry counts it")),
    _s("w256_three", 32, 256, 0, THREE, 2500, 42),
    _s("w256_even", 32, 256, 0, THREE, 2400, 42),
    _s("w256_five", 32, 256, 0, FIVE, 600, 44),
    _s("w32", 32, 32, 0, THREE, 600, 25),
    _s("pos_only_loss", 32, 128, 0, FIVE, 600, 3, loss=(POS,),
       same_as=("dnerf", "the loss does not change the route: unused outputs' gradients are zero-filled")),
    _s("skip_opacity", 32, 128, 0, (POS, SCALES, ROT, SHS), 600, 41,
       same_as=("dnerf", "a non-contiguous head subset packs and runs like any other")),
    _s("rot_only", 32, 128, 0, (ROT,), 600, 21, same_as=("dnerf", "k = 1 is the same launches")),
    _s("dynerf_p1", 32, 128, 0, FIVE, 1, 3, same_as=("dnerf", "P does not change the route")),
    _s("dynerf_p65", 32, 128, 0, FIVE, 65, 49, same_as=("dnerf", "P does not change the route")),
    _s("bf16_dynerf", 32, 128, 0, FIVE, 600, 3, dtype="bf16"),
    _s("bf16_dnerf", 64, 64, 0, THREE, 2500, 9, dtype="bf16"),
    _s("bf16_w256", 32, 256, 0, THREE, 2500, 42, dtype="bf16"),
    _s("bf16_default", 128, 64, 1, THREE, 2500, 2, dtype="bf16"),
))
FP32 = [n for n, s in SCENES.items() if s.dtype == "fp32"]
BF16 = [n for n, s in SCENES.items() if s.dtype == "bf16"]


# ---- the route restatement -------------------------------------------------------------------------------------------

ENTRIES = ("feature_relu_forward", "feature_relu_forward:with_hb", "feature_relu_backward", "heads_block_forward",
           "heads_block_forward_bf16", "heads_forward", "heads_backward", "mlp_dw_f32", "mlp_dx_f32", "mlp_dw_bf16",
           "mlp_dx_bf16", "linear_dw", "gemm_f32", "sum_slices")
LEAVES = ("first:feature_relu", "first:feature_relu_hb", "first:linear", "first:deep",
          "fwd:block", "fwd:heads_forward", "fwd:addmm",
          "bwd:kernel+mfma", "bwd:kernel+rocblas", "bwd:torch+linear_dw", "bwd:torch",
          "dw:one_gemm", "dw:split+remainder", "dw:split_even",
          "bf16:dw_mfma", "bf16:dw_rocblas", "bf16:torch")
FIRST_LAYER_SHAPES = ((32, 128), (48, 128), (64, 64), (32, 64))  # (feat_dim, W) the fused first layer is built for
K_CHUNK = 1024


def _split_k(P, c, leaves):
    """dW = dy^T x over P rows on rocBLAS: the chunk is the largest multiple of 8 in [3/4, 2] K_CHUNK that divides P,
    else K_CHUNK; fewer than two chunks: one GEMM; else one batched GEMM, one more for a remainder, one sum."""
    chunk = next((d for d in range(2 * K_CHUNK, (3 * K_CHUNK) // 4 - 1, -8) if P % d == 0), K_CHUNK)
    S = P // chunk
    if S < 2:
        leaves.add("dw:one_gemm")
        c["gemm_f32"] += 1
    else:
        rem = P - S * chunk
        leaves.add("dw:split+remainder" if rem else "dw:split_even")
        c["gemm_f32"] += 2 if rem else 1
        c["sum_slices"] += 1


def route(feat_dim, W, depth, head_widths, dtype, P):
    """(call counts per ENTRIES, the LEAVES of the rule taken) for one training forward plus backward on the GPU
    with the fused heads."""
    assert P >= 1 and 1 <= len(head_widths) <= 5 and dtype in ("fp32", "bf16")
    c, leaves = dict.fromkeys(ENTRIES, 0), set()
    k, ns = len(head_widths), list(head_widths)
    # feature_out: one Linear (defor_depth <= 1) of a served shape is one fused pass with the heads' ReLU
    if depth <= 1 and (feat_dim, W) in FIRST_LAYER_SHAPES:
        leaves.add("first:feature_relu_hb" if dtype == "bf16" else "first:feature_relu")
        c["feature_relu_forward"] += 1
        c["feature_relu_forward:with_hb"] += dtype == "bf16"
        c["feature_relu_backward"] += 1
    else:
        leaves.add("first:linear" if depth <= 1 else "first:deep")
    if dtype == "bf16":
        # the HIP bf16 block for W in {64, 128} and heads of at most 16 or exactly 48 outputs, else torch bf16 ops
        if W in (64, 128) and all(n <= 16 or n == 48 for n in ns):
            c["heads_block_forward_bf16"] += 1
            c["heads_backward"] += 1
            if W == 128:
                leaves.add("bf16:dw_mfma")
                c["mlp_dw_bf16"] += 1
            else:
                leaves.add("bf16:dw_rocblas")
                _split_k(P, c, leaves)
            c["mlp_dx_bf16"] += 1  # k W is a multiple of 64 for both widths
        else:
            leaves.add("bf16:torch")
        return c, leaves
    # forward: both layers in one pass for W in {64, 128}; W = 256: the second layers in one pass when their weights
    # fit 64 KiB of LDS; else an addmm per head
    if W in (64, 128) and all(n <= 64 for n in ns):
        leaves.add("fwd:block")
        c["heads_block_forward"] += 1
    elif W == 256 and all(n <= 64 for n in ns) and sum(ns) * (W + 4) * 4 <= 64 * 1024:
        leaves.add("fwd:heads_forward")
        c["heads_forward"] += 1
    else:
        leaves.add("fwd:addmm")
    # backward: one pass over a when k W <= 768 and every head has at most 16 outputs (48 too up to W = 128)
    if W in (64, 128, 256) and k * W <= 768 and all(n <= 16 or (n == 48 and W <= 128) for n in ns):
        c["heads_backward"] += 1
        if W in (64, 128):
            leaves.add("bwd:kernel+mfma")
            c["mlp_dw_f32"] += 1
            c["mlp_dx_f32"] += 1
        else:
            leaves.add("bwd:kernel+rocblas")
            _split_k(P, c, leaves)  # dW1
            c["gemm_f32"] += 1      # dx
    else:
        # torch: heads of at most 8 outputs share one linear_dw launch (W in {64, 128, 256}), the others and the
        # first layers take the split-K weight gradient; dx is torch's
        small = [n for n in ns if n <= 8] if W in (64, 128, 256) else []
        leaves.add("bwd:torch+linear_dw" if small else "bwd:torch")
        c["linear_dw"] += 1 if small else 0
        for _ in range(k - len(small)):
            _split_k(P, c, leaves)
        _split_k(P, c, leaves)  # dW1
    return c, leaves


def expected_calls(feat_dim, W, depth, head_widths, dtype, P):
    return route(feat_dim, W, depth, head_widths, dtype, P)[0]


def scene_route(name):
    s = SCENES[name]
    return route(s.feat_dim, s.W, s.depth, [HEAD_N[i] for i in s.heads], s.dtype, s.P)


# ---- networks, inputs, runners ---------------------------------------------------------------------------------------

_FIELD = {32: (16, [1, 2]), 64: (32, [1, 2]), 128: (32, [1, 2, 3, 4])}  # feat_dim: (features per level, levels)


def hyper(s):
    from gs4d_train import config
    ocd, multires = _FIELD[s.feat_dim]
    flags = {f: i not in s.heads for i, f in enumerate(FLAGS)}
    return config.model_hidden_params(
        net_width=s.W, defor_depth=s.depth, multires=multires, mlp_dtype=s.dtype,
        kplanes_config={"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": ocd,
                        "resolution": [8, 8, 8, 5]}, **flags)


def build(s, device="cpu", fused=False):
    """The scene's Deformation, drawn on the CPU from its seed, on `device`; fused: the HIP field and heads."""
    from gs4d_train.deformation import Deformation
    h = hyper(s)
    g = torch.Generator().manual_seed(1000 + s.seed)
    net = Deformation(W=h.net_width, D=h.defor_depth, args=h)
    assert net.grid.feat_dim == s.feat_dim
    with torch.no_grad():
        for level in net.grid.grids:
            for p in level:
                p.copy_(torch.rand(p.shape, generator=g) * 0.4 + 0.1)
        for m in net.modules():
            if isinstance(m, torch.nn.Linear):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / m.in_features ** 0.5)
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
    net = net.to(device)
    net.grid.fused = net.fused_heads = fused
    return net


def inputs(s, device="cpu", dtype=torch.float32, seed=None):
    """(the five inputs, the five upstream gradients, time) of the scene"""
    g = torch.Generator().manual_seed(s.seed if seed is None else seed)
    rn = lambda *sh: torch.randn(*sh, generator=g)
    P = s.P
    xyz = torch.rand(P, 3, generator=g) * 2.4 - 1.2
    ins = [xyz, rn(P, 3), rn(P, 4), rn(P, 1), rn(P, 16, 3)]
    ups = [rn(P, 3), rn(P, 3), rn(P, 4), rn(P, 1), rn(P, 16, 3)]
    to = lambda t: t.to(device=device, dtype=dtype)
    time = torch.full((P, 1), float(np.float32(0.37)), dtype=dtype, device=device)
    return [to(t) for t in ins], [to(t) for t in ups], time


def reference_net(net, dtype=torch.float64):
    """The unfused torch graph of the same parameters in `dtype`: F.grid_sample and the separate heads."""
    ref = copy.deepcopy(net).to(dtype)
    ref.grid.fused = ref.fused_heads = False
    ref.mlp_dtype = "fp32"
    return ref


def run(net, s, dtype=torch.float32, zero=True, seed=None, rows=None):
    """One forward plus backward of sum(out * upstream) over the scene's loss heads.  -> ({head: its deformed
    output} for every active head, {name: gradient} for every parameter that received one and "xyz").
    zero=False keeps the parameters' .grad (accumulation).  rows: an index tensor; the loss reads those rows only."""
    dev = next(net.parameters()).device
    ins, ups, time = inputs(s, dev, dtype, seed)
    ins[0].requires_grad_(True)
    if zero:
        net.zero_grad(set_to_none=True)
    outs = net(*ins, time)
    loss = 0
    for i in s.loss:
        prod = outs[i] * ups[i]
        loss = loss + (prod[rows] if rows is not None else prod).sum()
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
    grads["xyz"] = ins[0].grad.detach().clone()
    return {HEADS[i]: outs[i].detach() for i in s.heads}, grads


def preactivations(net, s, dtype=torch.float64):
    """[(name, z, sum of |terms| of z)] for every ReLU input of the unfused graph of `net` in `dtype`: each Linear of
    feature_out (its last output meets the heads' leading ReLU) and each active head's first layer."""
    ref = reference_net(net, dtype)
    dev = next(ref.parameters()).device
    ins, _, time = inputs(s, dev, dtype)
    out = []
    with torch.no_grad():
        x = ref.grid(ins[0], time)
        for j, m in enumerate(ref.feature_out):
            if isinstance(m, torch.nn.Linear):
                z = m(x)
                out.append((f"feature_out.{j}", z, x.abs() @ m.weight.abs().t() + m.bias.abs()))
                x = torch.relu(z)
        for i in s.heads:
            m = getattr(ref, HEADS[i])[1]
            out.append((f"{HEADS[i]}.1", m(x), x.abs() @ m.weight.abs().t() + m.bias.abs()))
    return out


def rounding_ratio(net, s):
    """The largest |z32 - z64| / sum |terms| over the scene's ReLU inputs, fp32 unfused graph against fp64."""
    z64, z32 = preactivations(net, s, torch.float64), preactivations(net, s, torch.float32)
    return max(float(((a[1].double() - b[1]).abs() / b[2]).max()) for a, b in zip(z32, z64))


TIE_FACTOR = 8  # a kernel sums the same terms in another order: its error may be a few times the torch graph's


def tie_slack(net, s, ratio=None):
    """min over the ReLU inputs of |z| / margin, margin = TIE_FACTOR * ratio * sum |terms| per element: above 1, no
    fp32 evaluation within the margin takes the other side of a ReLU than the fp64 graph."""
    ratio = rounding_ratio(net, s) if ratio is None else ratio
    return min(float((z.abs() / (TIE_FACTOR * ratio * t)).min()) for _, z, t in preactivations(net, s))


def find_seed(name, tries=64):
    """The seed of the first `tries` with the largest tie slack (how the committed seeds were chosen)."""
    s = SCENES[name]
    best = max(range(tries), key=lambda sd: tie_slack(build(s._replace(seed=sd)), s._replace(seed=sd)))
    return best, tie_slack(build(s._replace(seed=best)), s._replace(seed=best))


def flipped_rows(net, s):
    """The rows on which any ReLU input has another sign in the fp32 unfused graph than in the fp64 one."""
    dev = next(net.parameters()).device
    bad = torch.zeros(s.P, dtype=torch.bool, device=dev)
    for a, b in zip(preactivations(net, s, torch.float32), preactivations(net, s, torch.float64)):
        bad |= ((a[1] > 0) != (b[1] > 0)).any(1)
    return bad


def sum_terms(net, s):
    """{name: sum of |terms|} in fp64 for the MLP's weight and bias gradients (|dy|^T |x|, sum |dy|) and the head
    outputs (|x| |W|^T + |b| + |base|), from the fp64 unfused graph's own intermediates."""
    ref = reference_net(net)
    dev = next(ref.parameters()).device
    ins, ups, time = inputs(s, dev, torch.float64)
    seen, hooks = {}, []
    for name, m in ref.named_modules():
        if isinstance(m, torch.nn.Linear):
            def fwd(mod, args, out, name=name):
                seen[name] = [args[0].detach(), None]
                out.register_hook(lambda g, name=name: seen[name].__setitem__(1, g.detach()))
            hooks.append(m.register_forward_hook(fwd))
    outs = ref(*ins, time)
    sum((outs[i] * ups[i]).sum() for i in s.loss).backward()
    for h in hooks:
        h.remove()
    terms = {}
    for name, (x, dy) in seen.items():
        if dy is not None:
            terms[name + ".weight"] = dy.abs().t() @ x.abs()
            terms[name + ".bias"] = dy.abs().sum(0)
    for i in s.heads:
        m = getattr(ref, HEADS[i])[3]
        x = seen[HEADS[i] + ".3"][0]
        t = x.abs() @ m.weight.detach().abs().t() + m.bias.detach().abs()
        terms[HEADS[i]] = t.reshape(ins[i].shape) + ins[i].detach().abs()
    return terms


# ---- the comparison ---------------------------------------------------------------------------------------------------

FACTOR, FLOOR, TERMS_BAR = 4.0, 1e-6, 1e-5


def rel_max(got, want):
    """max |got - want| / max |want| (inf for a non-finite result)"""
    err = (got.double() - want).abs()
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    return float(err.max()) / max(float(want.abs().max()), 1e-300)


def compare(got, control, want, terms=None, flipped=None):
    """Every tensor of `want` (fp64) must exist in `got` with e_got <= max(FACTOR e_control, FLOOR), e = max error
    over max |want|; a tensor named in `terms` may instead lie within TERMS_BAR terms[name] elementwise.  Tensors that
    `got` has beyond `want` (the zero fill of an output the loss does not read) must be exactly zero.
    -> ({name: (e_got, e_control)}, [failure messages])."""
    figures, failures = {}, []
    for k in want:
        if k not in got or k not in control:
            failures.append(f"{k}: missing")
            continue
        if got[k].shape != want[k].shape:
            failures.append(f"{k}: shape {tuple(got[k].shape)}, reference {tuple(want[k].shape)}")
            continue
        e_f, e_u = rel_max(got[k], want[k]), rel_max(control[k], want[k])
        figures[k] = (e_f, e_u)
        if e_f <= max(FACTOR * e_u, FLOOR):
            continue
        err = (got[k].double() - want[k]).abs()
        if terms is not None and k in terms and bool((err <= TERMS_BAR * terms[k]).all()):
            continue
        idx = np.unravel_index(int(torch.nan_to_num(err, nan=float("inf")).argmax()), err.shape) if err.dim() else ()
        msg = (f"{k}{list(map(int, idx))}: got {float(got[k][idx]):.9g}, reference {float(want[k][idx]):.9g}; "
               f"e_f {e_f:.3e} > max({FACTOR:g} x e_u {e_u:.3e}, {FLOOR:g})")
        if flipped is not None:
            per_row = err.dim() >= 1 and err.shape[0] == flipped.shape[0] and not k.endswith((".weight", ".bias"))
            if per_row:
                msg += f"; a ReLU input of row {int(idx[0])} changed sign in fp32: {bool(flipped[idx[0]])}"
            else:
                msg += f"; rows with a ReLU input that changed sign in fp32: {int(flipped.sum())} of {flipped.numel()}"
        failures.append(msg)
    for k in got:
        if k not in want and bool((got[k] != 0).any()):
            failures.append(f"{k}: the reference has no gradient here, got max |.| {float(got[k].abs().max()):.3e}")
    return figures, failures


def rel_l2(got, want):
    return float((got.double() - want).norm() / want.norm().clamp_min(1e-300))
