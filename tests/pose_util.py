"""What the pose tests compare against: lib/pose_utils.py restated with a dtype argument.  The reference cannot run in float64
(torch.zeros / torch.eye at pose_utils.py:45,55,63 are float32); this can, and at float32 it performs the reference's
operations in the reference's order (tests/test_pose_utils_abi.py pins both to the live reference on the CPU), so its
float32 run stands for "the fp32 reference" where the reference's files are not present - on the GPU machine.

Seeded case builders: unit and non-unit quaternions, s in [0.5, 2], t2 in [-0.5, 0.5], z0 in [-4, 4], both branches, and
non-contiguous views of the same values."""
import functools
import math

import numpy as np
import torch

from contract_util import strided  # noqa: F401  (the one copy of the view helpers; pu.strided as before)

EPS32 = 2.0 ** -23


# --------------------------------------------------------------------------- the six functions, in `dtype`
def rotation_rows(q):
    """[B,3,3]: row i is e_i + 2 (w u x e_i + u x (u x e_i)), q = (w, u) - polynomial in q, no normalisation."""
    b = q.shape[0]
    e = torch.eye(3, dtype=q.dtype).expand(b, 3, 3)
    u = q[:, None, 1:].expand(b, 3, 3)
    c1 = torch.cross(u, e, dim=2)
    c2 = torch.cross(u, c1, dim=2)
    return e + 2 * (q[:, :1, None] * c1 + c2)


def normalize(q):
    return q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def pose_to_matrix(z0, t2, s, q, camera_flipped, normalize_q=False, dtype=torch.float64):
    """(cam2world [B,4,4], focal [B] or None) in `dtype`; the inputs are cast, not detached (autograd works through it)."""
    t2, s, q = t2.to(dtype), s.to(dtype), q.to(dtype)
    if normalize_q:
        q = normalize(q)
    rows = rotation_rows(q)
    if z0 is not None:
        f = 1 + z0.to(dtype).exp()
        t3 = torch.cat([t2 / s[:, None], (f / s)[:, None]], dim=-1)
    else:
        t3 = torch.cat([t2, torch.ones_like(t2[:, :1]) * 10], dim=-1)
    shift = (t3[:, None, :] * rows).sum(dim=-1)
    top = torch.cat([rows, shift[:, :, None]], dim=2)
    if camera_flipped:
        top = top * torch.tensor([1, -1, -1, -1], dtype=dtype)
    bottom = torch.tensor([0, 0, 0, 1], dtype=dtype).expand(q.shape[0], 1, 4)
    mat = torch.cat([top, bottom], dim=1)
    if z0 is not None:
        return mat, f / 2
    return mat / s[:, None, None], None


def world2cam(cam2world, camera_flipped):
    """invert_space of the (un-flipped) matrix, in the matrix's dtype."""
    m = cam2world.clone()
    if camera_flipped:
        m[:, :3, 1:] = -m[:, :3, 1:]
    a = m[:, :3, :3] / m[:, 3:4, 3:4]
    shift = -(a * m[:, :3, 3:4]).sum(dim=1)
    out = torch.zeros_like(m)
    out[:, :3, :3] = a.transpose(1, 2)
    out[:, :3, 3] = shift
    out[:, 3, 3] = 1
    return out


def quaternion_of(m):
    """(q (w,x,y,z) float64 [4], branch) of one 4 x 4 numpy float64 matrix: branch 0 takes w from the trace, 1 + i takes
    component i of the vector part from the diagonal (pose_utils.py:73-95, the same tests in the same order)."""
    h = m[3, 3]
    t = ((m[0, 0] + m[1, 1]) + m[2, 2]) + h
    q = np.empty(4)
    if t > h:
        branch = 0
        q[:] = t, m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1]
    else:
        i = 1 if m[1, 1] > m[0, 0] else 0
        i = 2 if m[2, 2] > m[i, i] else i
        j, k = (i + 1) % 3, (i + 2) % 3
        branch = 1 + i
        t = m[i, i] - (m[j, j] + m[k, k]) + h
        q[0], q[1 + i], q[1 + j], q[1 + k] = m[k, j] - m[j, k], t, m[i, j] + m[j, i], m[k, i] + m[i, k]
    return q * (0.5 / math.sqrt(t * h)), branch


def matrix_to_pose(cam2world, focal, camera_flipped, dtype=torch.float64):
    """(z0 or None, t2, s, q, cond [B,13], branches): the algebra in `dtype`, the quaternion in float64 from the `dtype`
    world2cam matrix (as the reference: numpy float64 on its float32 matrix), everything returned in `dtype`."""
    m = cam2world.to(dtype)
    w = world2cam(m, camera_flipped)
    t3 = -w[:, :3, 3]
    if focal is not None:
        focal = focal.to(dtype)
        z0, z0_cond = torch.log(2 * focal - 1), torch.log(focal)
        s = 2 * focal / t3[:, 2]
    else:
        s = 1 / m[:, 3, 3]
        z0, z0_cond = None, torch.zeros_like(s)
    t2 = t3[:, :2] * s[:, None]
    qs, branches = zip(*(quaternion_of(x) for x in w.double().numpy()))
    q = torch.from_numpy(np.stack(qs)).to(dtype)
    cond = torch.cat([z0_cond[:, None], t2, s[:, None], w[:, :3, :3].flatten(1, 2)], dim=-1)
    return z0, t2, s, q, cond, list(branches)


def rotation_distance(p, q, dtype=torch.float64):
    p, q = p.to(dtype), q.to(dtype)
    if p.shape[-1] == 4:
        p, q = p[:, :3, :3] / p[:, 3:4, 3:4], q[:, :3, :3] / q[:, 3:4, 3:4]
    pqt = p @ q.transpose(-2, -1)
    trace = pqt[:, 0, 0] + pqt[:, 1, 1] + pqt[:, 2, 2]
    return torch.acos(((trace - 1) / 2).clamp(-1, 1)) / np.pi * 180


def pairwise_distance(cam2world, dtype=torch.float64):
    """[N,N] degrees, row i = distances of pose i to every pose (what perturb_poses forms one row at a time)."""
    n = cam2world.shape[0]
    return torch.stack([rotation_distance(cam2world[i:i + 1].expand(n, -1, -1), cam2world, dtype) for i in range(n)])


def nearest_by_angle(cam2world, target, dtype=torch.float64):
    """index [N]: the first j minimising |d(i, j) - target_i| with distances and the subtraction in `dtype`."""
    gap = (pairwise_distance(cam2world, dtype) - target.to(dtype)[:, None]).abs()
    return (gap == gap.min(dim=1, keepdim=True).values).float().argmax(dim=1)


def project(q, s, z0):
    """run.py:2307-2310 out of place, float32 as the reference runs it."""
    return torch.nn.functional.normalize(q, dim=-1), s.abs(), None if z0 is None else z0.clamp(-4, 4)


# --------------------------------------------------------------------------- cases
def random_quaternions(n, g, unit=True):
    q = torch.randn(n, 4, generator=g)
    q = q / q.norm(dim=-1, keepdim=True)
    return q if unit else q * (0.5 + 1.5 * torch.rand(n, 1, generator=g))


def axis_turns(degrees=(125.0, 150.0, 179.0)):
    """Unit quaternions of turns by more than 120 degrees about x, y and z, and about the diagonals between them: with the
    random ones, all four branches of the quaternion extraction."""
    axes = torch.tensor([[1., 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1], [0.2, 1, 0.1], [0.1, 0.2, 1], [1, 0.1, 0.2]])
    axes = axes / axes.norm(dim=-1, keepdim=True)
    out = [torch.cat([torch.full((len(axes), 1), math.cos(math.radians(d) / 2)), axes * math.sin(math.radians(d) / 2)], dim=1)
           for d in degrees]
    return torch.cat(out).float()


@functools.lru_cache(maxsize=None)
def case(b, perspective, unit=True, seed=0, turns=False):
    """Float32 CPU tensors q [b,4], t2 [b,2], s [b], z0 [b] or None (never modified: shared between tests).  turns: the
    first rows of q are axis_turns()."""
    g = torch.Generator().manual_seed(1000 * seed + 10 * b + 2 * perspective + unit)
    q = random_quaternions(b, g, unit)
    if turns:
        t = axis_turns()[:b]
        q = torch.cat([t, q[len(t):]])
    t2 = torch.rand(b, 2, generator=g) - 0.5
    s = 0.5 + 1.5 * torch.rand(b, generator=g)
    z0 = torch.rand(b, generator=g) * 8 - 4 if perspective else None
    return dict(q=q.float(), t2=t2, s=s, z0=z0)


def rotations(n, g):
    """n random rotation matrices [n,3,3], float32 (rounded from float64)."""
    return rotation_rows(random_quaternions(n, g).double()).float()


def poses_4x4(n, seed):
    """cam2world-like [n,4,4] float32 with a non-unit element [3,3] (the orthographic branch's)."""
    c = case(n, False, seed=seed)
    return pose_to_matrix(None, c['t2'], c['s'], c['q'], False)[0].float()
