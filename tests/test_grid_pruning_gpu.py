"""GPU tests of gs4d_voxel_downsample (csrc/voxel.hip) and gs4d_train.pruning against the fp64 numpy restatement
in tests/voxel_refs.py.

What is compared: the voxel keys, read off the helper's sorted point keys at the runs the device's counts cut out;
M and the counts exactly; every point and colour element within ONE fp32 ulp of the helper's.  The ulp bound is
derived: both sides sum the same n fp32 values in fp64 and differ only in the order, so the sums differ by at most
about n 2^-53 relative to sum |x| -- many orders of magnitude below an fp32 ulp (2^-24) for any n here -- and the
two roundings to fp32 are equal or adjacent."""
import numpy as np
import pytest
import torch

import voxel_refs

pytestmark = pytest.mark.gpu


def _run(points, colors, voxel):
    from gs4d_train import _C
    dev = torch.device("cuda:0")
    p = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to(dev)
    c = None if colors is None else torch.from_numpy(np.ascontiguousarray(colors, dtype=np.float32)).to(dev)
    op, oc, cnt = _C.voxel_downsample(p, c, float(voxel))
    torch.cuda.synchronize()
    return op.cpu().numpy(), None if oc is None else oc.cpu().numpy(), cnt.cpu().numpy()


def _check(points, colors, voxel):
    """Run the device downsample and hold it against the helper; returns (helper result, device result)."""
    keys, counts, want_p, want_c = voxel_refs.voxel_downsample(points, colors, voxel)
    got_p, got_c, got_n = _run(points, colors, voxel)
    assert got_n.dtype == np.int32 and got_p.dtype == np.float32
    assert got_p.shape == (len(keys), 3), (got_p.shape, len(keys))      # M
    assert np.array_equal(got_n.astype(np.int64), counts)               # the counts, exactly
    # the keys of the device's rows: its counts cut the helper's sorted keys into runs; every run must hold one
    # key, and the runs' keys are the helper's, ascending
    sk = voxel_refs.sorted_keys(points, voxel)
    ends = np.cumsum(got_n.astype(np.int64))
    assert ends[-1] == sk.size
    starts = ends - got_n
    assert np.array_equal(sk[starts], sk[ends - 1]) and np.array_equal(sk[starts], keys)
    assert np.all(np.diff(sk[starts]) > 0)
    d = voxel_refs.ulp_distance(got_p, want_p)
    print(f"N={len(points)} M={len(keys)} voxel={voxel:.6g} max count {counts.max()} point ulp max {d.max()}", end="")
    assert d.max() <= 1, d.max()
    if colors is None:
        assert got_c is None
    else:
        dc = voxel_refs.ulp_distance(got_c, want_c)
        print(f" colour ulp max {dc.max()}", end="")
        assert got_c.shape == got_p.shape and dc.max() <= 1, dc.max()
    print()
    return (keys, counts, want_p, want_c), (got_p, got_c, got_n)


def _bbox_voxel(points):
    p = np.asarray(points)
    return float(np.linalg.norm(p.max(axis=0) - p.min(axis=0)) / 100.0)


def test_one_point_and_two_points_in_one_voxel():
    p = np.array([[0.3, -1.7, 2.9]], np.float32)
    c = np.array([[0.1, 0.5, 0.9]], np.float32)
    _, (gp, gc, gn) = _check(p, c, 0.25)
    assert np.array_equal(gp, p) and np.array_equal(gc, c) and gn.tolist() == [1]
    p2 = np.array([[0.30, 0.10, -0.20], [0.31, 0.12, -0.21]], np.float32)
    (_, counts, _, _), _ = _check(p2, np.array([[0, 0.25, 1], [1, 0.75, 0]], np.float32), 0.5)
    assert counts.tolist() == [2]


def test_identical_points_make_one_voxel_across_many_waves():
    p = np.tile(np.array([[0.123, -4.5, 7.25]], np.float32), (50_000, 1))
    c = np.tile(np.array([[0.2, 0.4, 0.6]], np.float32), (50_000, 1))
    (_, counts, _, _), (gp, gc, _) = _check(p, c, 0.05)
    assert counts.tolist() == [50_000]
    assert np.array_equal(gp, p[:1]) and np.array_equal(gc, c[:1])  # the mean of equal values is that value


def test_clustered_cloud_with_bbox_voxels():
    p, c = voxel_refs.clustered_cloud(20_001, seed=3, sigma=0.02)
    (keys, counts, _, _), _ = _check(p, c, _bbox_voxel(p))
    # voxels inside a wave, voxels across two waves and voxels with whole waves in their middle
    assert 1 < len(keys) < 20_001 and counts.min() == 1 and counts.max() > 128


def test_every_point_alone_in_its_voxel():
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(5)
    p = (g[rng.permutation(4096)] * 1.0 + rng.uniform(0.1, 0.4, (4096, 3))).astype(np.float32)
    (_, counts, _, _), _ = _check(p, rng.uniform(0, 1, (4096, 3)).astype(np.float32), 0.5)
    assert len(counts) == 4096 and counts.max() == 1


def test_lattice_with_points_on_voxel_faces():
    a = (np.arange(9) - 4) * 0.25
    p = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    (keys, counts, _, _), _ = _check(p, np.abs(p) * 0.5, 0.5)
    assert len(keys) == 125 and counts.min() == 1 and counts.max() == 8


def test_all_negative_coordinates():
    rng = np.random.default_rng(8)
    p = (-rng.uniform(5.0, 9.0, (3000, 3))).astype(np.float32)
    _check(p, rng.uniform(0, 1, (3000, 3)).astype(np.float32), 0.2)


def test_two_word_sort_path():
    rng = np.random.default_rng(9)
    p = rng.uniform(-1, 1, (2000, 3)).astype(np.float32)
    p[1000:] = p[:1000] + np.float32(1e-5)  # pairs that share a voxel, most of the time
    p = np.clip(p, -1, 1)
    sk = voxel_refs.sorted_keys(p, 1e-3)
    assert sk.max() >= 2 ** 32  # nx ny nz > 2^32: the keys need the high word
    (_, counts, _, _), _ = _check(p, rng.uniform(0, 1, (2000, 3)).astype(np.float32), 1e-3)
    assert counts.max() >= 2


def test_without_colours():
    p, _ = voxel_refs.clustered_cloud(5000, seed=4)
    _check(p, None, _bbox_voxel(p))


def test_a_nan_point_and_an_axis_of_2_21_voxels_are_refused():
    from gs4d_train import _C
    p, c = voxel_refs.clustered_cloud(1000, seed=6)
    p[517, 1] = np.nan
    with pytest.raises(RuntimeError, match=r"voxel_downsample:.*\(status 1\)"):
        _C.voxel_downsample(torch.from_numpy(p).cuda(), torch.from_numpy(c).cuda(), 0.1)
    far = torch.tensor([[0.0, 0.0, 0.0], [2.1, 0.0, 0.0]], device="cuda")
    with pytest.raises(RuntimeError, match=r"voxel_downsample:.*2\^21.*\(status 1\)"):
        _C.voxel_downsample(far, None, 1e-6)
    # the library is usable afterwards
    _check(np.array([[0.0, 0.0, 0.0], [2.1, 0.0, 0.0]], np.float32), None, 1e-3)


def test_two_calls_are_bitwise_equal_and_a_permutation_changes_nothing():
    p, c = voxel_refs.clustered_cloud(20_001, seed=7)
    v = _bbox_voxel(p)
    a, b = _run(p, c, v), _run(p, c, v)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    perm = np.random.default_rng(1).permutation(len(p))
    q = _run(p[perm], c[perm], v)
    assert np.array_equal(q[2], a[2])  # the same counts, so (with ascending rows) the same keys
    sk = voxel_refs.sorted_keys(p[perm], v)
    assert np.array_equal(sk, voxel_refs.sorted_keys(p, v))
    assert voxel_refs.ulp_distance(q[0], a[0]).max() <= 1 and voxel_refs.ulp_distance(q[1], a[1]).max() <= 1
    want = voxel_refs.voxel_downsample(p[perm], c[perm], v)
    assert voxel_refs.ulp_distance(q[0], want[2]).max() <= 1 and voxel_refs.ulp_distance(q[1], want[3]).max() <= 1


def test_grid_pruning_with_motion_is_static_then_dynamic():
    from gs4d_train import pruning
    p, c = voxel_refs.clustered_cloud(6000, seed=11)
    motion = np.where(np.arange(6000) % 2 == 0, 0.2, 0.9)
    gp, gc, gm = pruning.grid_pruning_with_motion(p, c, motion_prob=motion, cameras=None)
    stat, dyn = motion <= 0.7, motion > 0.7
    vs = pruning.adaptive_voxel_size(p[stat], None, scale_factor=4.0)
    vd = pruning.adaptive_voxel_size(p[dyn], None, scale_factor=3.0)
    assert vs != vd
    ws, wd = voxel_refs.voxel_downsample(p[stat], c[stat], vs), voxel_refs.voxel_downsample(p[dyn], c[dyn], vd)
    ms, md = len(ws[0]), len(wd[0])
    assert gp.is_cuda and gp.shape == (ms + md, 3) and gc.shape == (ms + md, 3)
    assert gm.cpu().numpy().tolist() == [0.0] * ms + [1.0] * md
    assert voxel_refs.ulp_distance(gp.cpu().numpy(), np.concatenate([ws[2], wd[2]])).max() <= 1
    assert voxel_refs.ulp_distance(gc.cpu().numpy(), np.concatenate([ws[3], wd[3]])).max() <= 1
    # without motion_prob: one size, no flags
    one_p, one_c, none = pruning.grid_pruning_with_motion(p, c, cameras=None)
    w = voxel_refs.voxel_downsample(p, c, pruning.adaptive_voxel_size(p, None, scale_factor=3.5))
    assert none is None and one_p.shape == (len(w[0]), 3)
    assert voxel_refs.ulp_distance(one_p.cpu().numpy(), w[2]).max() <= 1


def _model():
    from gs4d_train import config
    from gs4d_train.gaussians import GaussianModel
    hyper, opt = config.dynerf()
    opt.iterations = 0
    torch.manual_seed(7)
    return GaussianModel(3, hyper, fused=True), hyper, opt


def test_initialize_with_grid_pruning_trains():
    from gs4d_train import pruning
    from gs4d_train.synthetic import make_point_cloud, make_training_views
    from gs4d_train.train import train_step
    pts, cols = make_point_cloud(20_000, seed=5)
    views = make_training_views(3, 64, 64, seed=6)
    cams = [cam for cam, _ in views]
    g, hyper, opt = _model()
    pruning.initialize(g, pts, cols, 1.0, cameras=cams, use_grid_pruning=True)
    voxel = pruning.adaptive_voxel_size(pts, cams[:10], scale_factor=3.5)
    keys, _, want_p, _ = voxel_refs.voxel_downsample(pts, cols, voxel)
    P = g._xyz.shape[0]
    print(f"initialize: 20000 -> {P} points at voxel {voxel:.6g}")
    assert P == len(keys) and 0 < P < 20_000
    assert voxel_refs.ulp_distance(g._xyz.detach().cpu().numpy(), want_p).max() <= 1
    aabb = g._deformation.deformation_net.grid.aabb.detach().cpu().numpy()
    assert np.array_equal(aabb, np.stack([pts.max(axis=0), pts.min(axis=0)]))  # the UNPRUNED cloud's
    assert torch.isfinite(g._scaling).all()
    g.training_setup(opt)
    bg = torch.ones(3, device="cuda")
    for it in (1, 2, 3):
        loss = train_step(g, views[it - 1:it], opt, hyper, it, bg, stage="coarse")
        assert np.isfinite(float(loss)), (it, loss)


def test_initialize_without_grid_pruning_is_create_from_pcd():
    from gs4d_train import pruning
    from gs4d_train.synthetic import make_point_cloud
    pts, cols = make_point_cloud(5000, seed=5)
    a, _, _ = _model()
    pruning.initialize(a, pts, cols, 1.0, cameras=None, use_grid_pruning=False)
    b, _, _ = _model()
    b.create_from_pcd(pts, cols, 1.0)
    for name in ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity", "max_radii2D",
                 "_deformation_table"):
        assert torch.equal(getattr(a, name).detach(), getattr(b, name).detach()), name
    assert a.spatial_lr_scale == b.spatial_lr_scale == 1.0
