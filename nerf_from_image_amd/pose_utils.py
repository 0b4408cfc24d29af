"""Drop-in for the reference's lib/pose_utils.py (``from nerf_from_image_amd import pose_utils``): the same names, argument
order and return values, with the per-pose algebra as HIP kernels (csrc/nfi_pose.inc, thread = image, one launch per call).

* ``pose_to_matrix`` (48-70) is ONE autograd node (autograd.PoseToMatrix): one launch forward, one backward, where the
  reference runs some two dozen small launches each way.  ``normalize=True`` takes ``F.normalize(q, dim=-1)`` of
  run.py:2257-2262 into the same launch; with the default the behaviour is the reference's.
* ``matrix_to_pose`` (98-121) stays on the device: the reference copies the batch to the host and loops over it in numpy.
* ``perturb_poses`` (159-174) draws its N targets on the host from the reference's seeded generator, then selects all N
  indices in one launch (the reference: N rounds with two host reads each).
* ``project_pose_`` is new: the three in-place fix-ups after an optimiser step (run.py:2307-2310) in one launch.
* ``matrix_to_quaternion`` (73-95) stays a host numpy function: the data loaders call it on the CPU.

Tensor arguments live on the GPU (a CPU tensor raises RuntimeError: no CPU path).  The kernels work in float64 on the
float32 inputs and round once, so they agree with the reference to its own rounding error, not bit for bit.
"""
import math

import numpy as np
import torch

from . import ops
from .augment import invert_space          # noqa: F401  (lib/pose_utils.py:20-27, bit-identical tensor expressions)
from .autograd import PoseToMatrix


def quaternion_rotate_vector(q, v):
    """v [B,K,3] turned by the quaternions q [B,4] = (w, u): v + 2 (w u x v + u x (u x v)), lib/pose_utils.py:30-38.
    Tensor expressions, polynomial in q (a non-unit q is not normalised)."""
    assert q.shape[-1] == 4
    assert v.shape[-1] == 3
    w = q[:, None, :1]
    u = q[:, None, 1:].expand(-1, v.shape[1], -1)
    u_x_v = torch.cross(u, v, dim=2)
    return v + 2 * (w * u_x_v + torch.cross(u, u_x_v, dim=2))


def quaternion_to_matrix(q):
    """[B,3,3] whose ROW i is e_i turned by q (lib/pose_utils.py:41-45): the transpose of the usual column convention."""
    return quaternion_rotate_vector(q, torch.eye(3, device=q.device).expand(q.shape[0], 3, 3))


def pose_to_matrix(z0, t2, s, q, camera_flipped: bool, normalize=False):
    """(z0 [B] or None, t2 [B,2], s [B], q [B,4]) -> (cam2world [B,4,4], focal [B]), or (cam2world, None) when z0 is None
    (orthographic), lib/pose_utils.py:48-70.  normalize=True: q is normalised first, inside the launch (and its backward)."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (z0, t2, s, q)):
        return PoseToMatrix.apply(z0, t2, s, q, camera_flipped, normalize)
    return ops.pose_to_matrix(q, t2, s, z0, camera_flipped, normalize)


def matrix_to_quaternion(matrix):
    """Host, numpy float64 (lib/pose_utils.py:73-95): (w, x, y, z) of the rotation in the top-left 3 x 3 of a 4 x 4 matrix
    [[R, .], [0, h]].  The component of largest magnitude is taken from the diagonal and the other three from the
    off-diagonal sums and differences; the branch tests and the summation order are the reference's."""
    m = np.asarray(matrix, dtype=np.float64)[:4, :4]
    h = m[3, 3]
    pivot = ((m[0, 0] + m[1, 1]) + m[2, 2]) + h
    q = np.empty((4,))
    if pivot > h:
        q[:] = pivot, m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1]
    else:
        i = 1 if m[1, 1] > m[0, 0] else 0
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        pivot = m[i, i] - (m[j, j] + m[k, k]) + h
        q[0] = m[k, j] - m[j, k]
        q[1 + i], q[1 + j], q[1 + k] = pivot, m[i, j] + m[j, i], m[k, i] + m[i, k]
    return q * (0.5 / math.sqrt(pivot * h))


def matrix_to_pose(tform_cam2world, focal_length, camera_flipped: bool):
    """The inverse of pose_to_matrix (lib/pose_utils.py:98-121): (z0 or None, t2, s, R) as device tensors, no host copy."""
    assert not tform_cam2world.requires_grad
    focal = None if focal_length is None else focal_length.detach()
    return ops.matrix_to_pose(tform_cam2world, focal, camera_flipped)[:4]


def matrix_to_conditioning_vector(tform_cam2world, focal_length, camera_flipped: bool):
    """The discriminator's pose conditioning [B,13] (lib/pose_utils.py:124-145): (log focal or 0, t2, s, the world2cam
    rotation row by row).  No gradient: its callers hand it dataset poses."""
    focal = None if focal_length is None else focal_length.detach()
    return ops.matrix_to_pose(tform_cam2world.detach(), focal, camera_flipped, want_pose=False, want_cond=True)[4]


def rotation_matrix_distance(p, q):
    """Angle in degrees [B] between the rotations of p and q, [B,3,3] or [B,4,4] (lib/pose_utils.py:148-156).  A report's
    figure: it carries no gradient (run.py:2102, 2290 read it with .item())."""
    return ops.rotation_distance(p.detach(), q.detach())


def perturb_targets(n, avg_angle):
    """The reference's N target distances: N single draws from torch.Generator().manual_seed(1234), which one draw of N
    reproduces (tests/test_pose_utils_abi.py pins it), each times avg_angle * 2 in float32 as the reference forms it."""
    return torch.rand((n,), generator=torch.Generator().manual_seed(1234)) * avg_angle * 2


def perturb_poses(tform_cam2world, avg_angle, *extra_args):
    """Each pose (and its row of every extra argument that is not None) is replaced by the pose of the set whose angle to
    it is closest to a random target of mean avg_angle degrees (lib/pose_utils.py:159-174): one launch, one index tensor."""
    target = perturb_targets(tform_cam2world.shape[0], avg_angle).to(tform_cam2world.device)
    indices = ops.pose_nearest_by_angle(tform_cam2world.detach(), target).long()          # (an int32 index is widened per use)
    transformed_args = [arg[indices.to(arg.device)].clone() if arg is not None else None for arg in extra_args]
    return (tform_cam2world[indices].clone(), *transformed_args)


def project_pose_(R, s, z0=None):
    """After an optimiser step, in place (run.py:2307-2310): R <- F.normalize(R, dim=-1), s <- |s|, z0 <- clamp(z0, -4, 4)
    when given.  Parameters are changed through .data, like the reference does; returns None."""
    ops.pose_project_(R.data, s.data, None if z0 is None else z0.data)
