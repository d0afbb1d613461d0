"""Per-camera pose corrections for pose refinement (no counterpart in the reference, whose poses are constants).

A PoseRefiner holds, per camera, a rotation `rot` (axis-angle omega) and a translation `trans` (tau), both zero at the
start, that perturb the camera in ITS OWN frame:

    p_view' = R(omega) p_view + tau

The rasterizer's matrices act on row vectors (p_view = ([m, 1] V)[:3]), so V' = V D with D = [[R^T, 0], [tau, 1]].
tensors(camera) returns (V', V' projection_matrix, c'), differentiable in the two deltas, for render(...,
camera_grad=True, camera_tensors=...).  They are formed as the camera's own tensors plus a correction that is exactly
zero at zero deltas,

    V' = V + V E        Pm' = Pm + (V E) projection        c' = c - (tau R) A^T        E = D - I, A = V[:3, :3]

so an untouched refiner hands the rasterizer the camera's own values, and the centre needs no matrix inverse: the
view rotation A is orthonormal (camera.get_world2view2), hence c' = -(t R^T + tau) (A R^T)^-1 = c - (tau R) A^T.
R(omega) = I + a K + b K^2 (Rodrigues; K the cross-product matrix of omega) with a = sin(theta) / theta and
b = (1 - cos(theta)) / theta^2 evaluated as functions of theta^2 = omega . omega -- by their series below
theta^2 = 1e-2 -- so no square root is differentiated at omega = 0 and the Jacobian there is finite.
"""
import torch

_SERIES_BELOW = 1e-2  # theta^2; the first dropped terms are theta^8 / 9! and theta^8 / 10!: below 3e-14 here


def _rodrigues_coefficients(theta2):
    """(sin(theta) / theta, (1 - cos(theta)) / theta^2) as smooth functions of theta^2 >= 0"""
    small = theta2 < _SERIES_BELOW
    # each branch gets an argument on which it is finite, so the branch not taken adds no NaN to the gradient
    safe = torch.where(small, torch.ones_like(theta2), theta2)
    th = torch.sqrt(safe)
    s2 = torch.where(small, theta2, torch.zeros_like(theta2))
    a_series = 1.0 - s2 / 6.0 * (1.0 - s2 / 20.0 * (1.0 - s2 / 42.0))
    b_series = 0.5 - s2 / 24.0 * (1.0 - s2 / 30.0 * (1.0 - s2 / 56.0))
    a = torch.where(small, a_series, torch.sin(th) / th)
    b = torch.where(small, b_series, (1.0 - torch.cos(th)) / safe)
    return a, b


def rotation_minus_identity(omega):
    """R(omega) - I = a K + b K^2 for an axis-angle vector (3,): exactly zero at omega = 0"""
    x, y, z = omega[0], omega[1], omega[2]
    o = torch.zeros_like(x)
    K = torch.stack([torch.stack([o, -z, y]), torch.stack([z, o, -x]), torch.stack([-y, x, o])])
    a, b = _rodrigues_coefficients((omega * omega).sum())
    return a * K + b * (K @ K)


class PoseRefiner:
    """rot (n, 3) axis-angle and trans (n, 3), zero leaves on `device`; a camera's row is its `uid` (a camera without
    one uses row 0, which is only right for a single camera)."""

    def __init__(self, n_cameras, device, dtype=torch.float32):
        self.rot = torch.zeros(n_cameras, 3, device=device, dtype=dtype, requires_grad=True)
        self.trans = torch.zeros(n_cameras, 3, device=device, dtype=dtype, requires_grad=True)

    def parameters(self):
        return [self.rot, self.trans]

    def _row(self, camera):
        uid = getattr(camera, "uid", None)
        if uid is None:
            if self.rot.shape[0] != 1:
                raise ValueError("PoseRefiner: a camera without a uid can only use a one-camera refiner")
            return 0
        if not 0 <= int(uid) < self.rot.shape[0]:
            raise ValueError(f"PoseRefiner: camera uid {uid} outside the {self.rot.shape[0]} rows")
        return int(uid)

    def tensors(self, camera):
        """(viewmatrix', projmatrix', campos') of the camera under its row's deltas (module docstring)"""
        i = self._row(camera)
        dev, dt = self.rot.device, self.rot.dtype
        if hasattr(camera, "on_device") and dt == torch.float32:
            V, Pm, c = camera.on_device(dev)
        else:
            V, Pm, c = (camera.world_view_transform.to(dev, dt), camera.full_proj_transform.to(dev, dt),
                        camera.camera_center.to(dev, dt))
        proj = camera.projection_matrix.to(dev, dt)
        dR = rotation_minus_identity(self.rot[i])                       # R - I
        tau = self.trans[i]
        E = torch.cat([torch.cat([dR.T, torch.zeros(3, 1, device=dev, dtype=dt)], 1),
                       torch.cat([tau, torch.zeros(1, device=dev, dtype=dt)]).unsqueeze(0)], 0)
        dV = V @ E
        A = V[:3, :3]
        c_new = c - (tau + tau @ dR) @ A.T
        return V + dV, Pm + dV @ proj, c_new

    def errors(self, i=0):
        """(|omega| in radians, |tau|) of row i, as Python floats"""
        return float(self.rot[i].detach().norm()), float(self.trans[i].detach().norm())
