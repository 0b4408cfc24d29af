"""CPU-side checks of the pose entries (csrc/nfi_pose.inc) at the C ABI, of the Python module's edges, and of the tests' own
reference: the header's prototypes and struct field orders, each entry's refusals - with a message, before any launch - no
CPU path, the reference's assert, perturb_poses' targets, and tests/pose_util.py against the LIVE lib/pose_utils.py on the
CPU (skipped where the reference's files are absent): values, autograd gradients, quaternions up to sign, the round trip."""
import ctypes
import re

import numpy as np
import pytest
import torch

from nerf_from_image_amd import _lib
from oracle import reference
import pose_util as pu

needs_reference = pytest.mark.skipif(not reference.available(), reason='reference sources not available (oracle/make_ref.py)')
U = 2.0 ** -24          # unit roundoff of float32

ENTRIES = {
    'nfi_pose_to_matrix_fwd': 'nfi_pose_args', 'nfi_pose_to_matrix_bwd': 'nfi_pose_args', 'nfi_matrix_to_pose': 'nfi_matrix_to_pose_args',
    'nfi_rotation_distance': 'nfi_rotation_distance_args', 'nfi_pose_nearest_by_angle': 'nfi_pose_nearest_args',
    'nfi_pose_project': 'nfi_pose_project_args'}
FIELDS = {
    'nfi_pose_args': ['n_images', 'camera_flipped', 'normalize_q', 'q', 't2', 's', 'z0', 'cam2world', 'focal', 'g_cam2world', 'g_focal',
                      'g_q', 'g_t2', 'g_s', 'g_z0'],
    'nfi_matrix_to_pose_args': ['n_images', 'camera_flipped', 'cam2world', 'focal', 'z0', 't2', 's', 'q', 'cond'],
    'nfi_rotation_distance_args': ['n_images', 'dim', 'p', 'q', 'degrees'],
    'nfi_pose_nearest_args': ['n_images', 'cam2world', 'target', 'index'],
    'nfi_pose_project_args': ['n_images', 'q', 's', 'z0']}
INTS = {'n_images', 'camera_flipped', 'normalize_q', 'dim'}


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    return _lib.load()


def test_entries_are_exported_with_the_header_prototypes(lib):
    src = _lib._strip_comments(open(_lib.HEADER).read())
    for name, struct in ENTRIES.items():
        m = re.search(r'(\w+)\s+%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m and m.group(1) == 'int' and [p.strip() for p in m.group(2).split(',')] == ['const %s* a' % struct, 'nfi_stream_t stream'], name
        assert _lib.FUNCTIONS[name] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == [ctypes.c_void_p, ctypes.c_void_p]
    assert lib.nfi_version() >= 103


def test_struct_field_order():
    for struct, names in FIELDS.items():
        assert [n for n, _ in _lib.STRUCT_FIELDS[struct]] == names, struct
        for n, kind in _lib.STRUCT_FIELDS[struct]:
            assert kind is (ctypes.c_int if n in INTS else ctypes.c_void_p), (struct, n)


def test_refusals_come_with_a_message_and_before_any_launch(lib):
    """Every pointer here is the number 16: a launch would fault, a refusal never reads it."""
    def refused(entry, word, base, **kw):
        a = _lib.make_args(ENTRIES[entry], **dict(base, **kw))
        rc, msg = getattr(lib, entry)(ctypes.byref(a), None), lib.nfi_last_error()
        assert rc == -1 and word in msg, (entry, kw, word, rc, msg)

    for entry in ENTRIES:
        assert getattr(lib, entry)(None, None) == -1 and b'null argument struct' in lib.nfi_last_error(), entry

    fwd = dict(n_images=3, q=16, t2=16, s=16, z0=16, cam2world=16, focal=16)
    for n in (0, -2):
        refused('nfi_pose_to_matrix_fwd', b'n_images', fwd, n_images=n)
    for missing in ('q', 't2', 's', 'cam2world'):
        refused('nfi_pose_to_matrix_fwd', b'null', fwd, **{missing: None})
    refused('nfi_pose_to_matrix_fwd', b'focal without z0', fwd, z0=None)

    bwd = dict(n_images=3, q=16, t2=16, s=16, z0=16, g_cam2world=16, g_focal=16, g_q=16, g_t2=16, g_s=16, g_z0=16)
    refused('nfi_pose_to_matrix_bwd', b'n_images', bwd, n_images=0)
    for missing in ('q', 't2', 's', 'g_cam2world'):
        refused('nfi_pose_to_matrix_bwd', b'null', bwd, **{missing: None})
    refused('nfi_pose_to_matrix_bwd', b'without z0', bwd, z0=None, g_focal=None)
    refused('nfi_pose_to_matrix_bwd', b'without z0', bwd, z0=None, g_z0=None)
    refused('nfi_pose_to_matrix_bwd', b'no gradient to write', bwd, g_q=None, g_t2=None, g_s=None, g_z0=None)

    m2p = dict(n_images=3, cam2world=16, focal=16, z0=16, t2=16, s=16, q=16, cond=16)
    refused('nfi_matrix_to_pose', b'n_images', m2p, n_images=0)
    refused('nfi_matrix_to_pose', b'null cam2world', m2p, cam2world=None)
    refused('nfi_matrix_to_pose', b'z0 without focal', m2p, focal=None)
    refused('nfi_matrix_to_pose', b'no output', m2p, z0=None, t2=None, s=None, q=None, cond=None)

    dist = dict(n_images=3, dim=4, p=16, q=16, degrees=16)
    refused('nfi_rotation_distance', b'n_images', dist, n_images=-1)
    for dim in (0, 2, 5, 16):
        refused('nfi_rotation_distance', b'dim must be 3 or 4', dist, dim=dim)
    for missing in ('p', 'q', 'degrees'):
        refused('nfi_rotation_distance', b'null', dist, **{missing: None})

    near = dict(n_images=3, cam2world=16, target=16, index=16)
    refused('nfi_pose_nearest_by_angle', b'n_images', near, n_images=0)
    for missing in ('cam2world', 'target', 'index'):
        refused('nfi_pose_nearest_by_angle', b'null', near, **{missing: None})

    proj = dict(n_images=3, q=16, s=16, z0=16)
    refused('nfi_pose_project', b'n_images', proj, n_images=0)
    for missing in ('q', 's'):
        refused('nfi_pose_project', b'null', proj, **{missing: None})
    with pytest.raises(RuntimeError, match='focal without z0'):
        _lib.call_struct('nfi_pose_to_matrix_fwd', 'nfi_pose_args', 0, **dict(fwd, z0=None))


def test_no_cpu_path():
    from nerf_from_image_amd import ops, pose_utils
    c = pu.case(3, True)
    m = pu.poses_4x4(3, 0)
    q, s, z0 = c['q'].clone(), c['s'].clone(), c['z0'].clone()
    calls = [lambda: pose_utils.pose_to_matrix(c['z0'], c['t2'], c['s'], c['q'], False),
             lambda: pose_utils.pose_to_matrix(None, c['t2'], c['s'], c['q'].clone().requires_grad_(), True, normalize=True),
             lambda: pose_utils.matrix_to_pose(m, None, False), lambda: pose_utils.matrix_to_pose(m, c['s'], True),
             lambda: pose_utils.matrix_to_conditioning_vector(m, None, False), lambda: pose_utils.rotation_matrix_distance(m, m),
             lambda: pose_utils.rotation_matrix_distance(m[:, :3, :3], m[:, :3, :3]), lambda: pose_utils.perturb_poses(m, 10.0, None, s),
             lambda: pose_utils.project_pose_(q, s, z0), lambda: pose_utils.project_pose_(q, s),
             lambda: ops.pose_to_matrix_bwd(m, None, c['q'], c['t2'], c['s']), lambda: ops.pose_nearest_by_angle(m, s)]
    for i, call in enumerate(calls):
        with pytest.raises(RuntimeError, match='GPU'):
            call()
            pytest.fail('call %d ran on the CPU' % i)
    assert torch.equal(q, c['q']) and torch.equal(s, c['s']) and torch.equal(z0, c['z0'])


def test_matrix_to_pose_keeps_the_reference_assert():
    from nerf_from_image_amd import pose_utils
    with pytest.raises(AssertionError):
        pose_utils.matrix_to_pose(pu.poses_4x4(2, 0).requires_grad_(), None, False)


@pytest.mark.parametrize('n', [1, 2, 65, 300])
def test_perturb_targets_are_n_single_draws(n):
    """lib/pose_utils.py:162-168 draws torch.rand((1,)) once per pose from one seeded generator and multiplies by avg_angle * 2
    in float32; the module draws all n at once."""
    from nerf_from_image_amd import pose_utils
    g = torch.Generator().manual_seed(1234)
    singles = [(torch.rand((1,), generator=g) * 7.5 * 2).item() for _ in range(n)]
    got = pose_utils.perturb_targets(n, 7.5)
    assert got.dtype == torch.float32 and got.device.type == 'cpu' and got.tolist() == singles


def test_host_matrix_to_quaternion_equals_the_restatement():
    from nerf_from_image_amd import pose_utils
    c = pu.case(40, True, turns=True)
    mats = pu.matrix_to_pose(pu.pose_to_matrix(c['z0'], c['t2'], c['s'], c['q'], False)[0], None, False)
    w = pu.world2cam(pu.pose_to_matrix(c['z0'], c['t2'], c['s'], c['q'], False)[0], False).numpy()
    assert set(mats[5]) == {0, 1, 2, 3}
    for m, q in zip(w, mats[3].numpy()):
        assert np.array_equal(pose_utils.matrix_to_quaternion(m), q)
        assert np.array_equal(pose_utils.matrix_to_quaternion(m.tolist()), q)


# --------------------------------------------------------------------------- the restatement against the live reference
CASES = [(b, persp, flipped, unit) for b in (1, 3, 33) for persp in (True, False) for flipped in (False, True) for unit in (True, False)]


def forward_scale(c):
    """The largest magnitude an intermediate of pose_to_matrix reaches: (1 + 2 |q|^2) for a rotation entry before the
    cancellation against e_i, times the 1-norm of t3 for the translation's three-term sum, times 1/s where the orthographic
    branch divides."""
    q2 = float((c['q'].double() ** 2).sum(-1).max())
    s = c['s'].double()
    if c['z0'] is not None:
        t3 = torch.cat([c['t2'].double() / s[:, None], ((1 + c['z0'].double().exp()) / s)[:, None]], dim=-1)
        k = 1.0
    else:
        t3 = torch.cat([c['t2'].double(), torch.full((len(s), 1), 10.0, dtype=torch.float64)], dim=-1)
        k = float((1 / s).max())
    return (1 + 2 * q2) * max(1.0, float(t3.abs().sum(-1).max())) * k


@needs_reference
def test_restatement_against_the_live_reference_forward():
    """Bound: an entry of the result is reached from the float32 inputs by at most 12 roundings in sequence (two cross
    products of a multiply and a subtract each, w * uv, the add, the doubling is exact, + e_i, exp, two divisions by s,
    the product with t3, two adds of the three-term sum, the division by s), each of relative size u = 2^-24 of an
    intermediate no larger than forward_scale; the float64 side adds nothing visible.  So |fp32 - fp64| <= 12 u scale; the
    test allows 16 u scale.  At float32 the restatement itself must BE the reference: same operations, same order, same bits."""
    ref = reference.modules().pose_utils
    worst = 0.0
    for b, persp, flipped, unit in CASES:
        c = pu.case(b, persp, unit)
        mat, focal = ref.pose_to_matrix(c['z0'], c['t2'], c['s'], c['q'], flipped)
        m64, f64 = pu.pose_to_matrix(c['z0'], c['t2'], c['s'], c['q'], flipped)
        m32, f32 = pu.pose_to_matrix(c['z0'], c['t2'], c['s'], c['q'], flipped, dtype=torch.float32)
        tol = 16 * U * forward_scale(c)
        err = float((mat.double() - m64).abs().max())
        worst = max(worst, err / tol)
        assert err <= tol, (b, persp, flipped, unit, err, tol)
        assert torch.equal(m32, mat)
        if persp:
            assert float((focal.double() - f64).abs().max()) <= 4 * U * float(f64.max()) and torch.equal(f32, focal)
        else:
            assert focal is None and f64 is None and f32 is None
        # the fused normalisation is F.normalize outside
        n64, _ = pu.pose_to_matrix(c['z0'], c['t2'], c['s'], c['q'], flipped, normalize_q=True)
        nref, _ = ref.pose_to_matrix(c['z0'], c['t2'], c['s'], torch.nn.functional.normalize(c['q'], dim=-1), flipped)
        unit_c = dict(c, q=torch.nn.functional.normalize(c['q'], dim=-1))
        assert float((nref.double() - n64).abs().max()) <= 16 * U * forward_scale(unit_c) + 4 * U * forward_scale(unit_c)
    print('float64 restatement against the live pose_to_matrix: worst error / bound %.3f' % worst)


@needs_reference
def test_restatement_against_the_live_reference_gradients():
    """Gradients of a random cotangent on (mat, focal) by float32 autograd of the reference against float64 autograd of the
    restatement.  Bound: the reverse sweep retraces the forward chain (12 roundings) once more per input and sums the 16
    cotangent entries, each term no larger than |g|max * forward_scale * max(1, 1/s)^2 * max(1, exp(z0)); so
    |fp32 - fp64| <= 2 * 12 * 16 u * that product, and a gradient that is exactly zero on one side is within it too."""
    ref = reference.modules().pose_utils
    worst = 0.0
    for b, persp, flipped, unit in CASES:
        c = pu.case(b, persp, unit)
        g = torch.Generator().manual_seed(b)
        g_mat, g_focal = torch.randn(b, 4, 4, generator=g), torch.randn(b, generator=g)
        names = ['q', 't2', 's'] + (['z0'] if persp else [])

        def grads(fn, dtype):
            leaves = {k: c[k].clone().to(dtype).requires_grad_() for k in names}
            mat, focal = fn(leaves.get('z0'), leaves['t2'], leaves['s'], leaves['q'], flipped)
            loss = (mat * g_mat.to(dtype)).sum() + ((focal * g_focal.to(dtype)).sum() if persp else 0)
            return torch.autograd.grad(loss, [leaves[k] for k in names])
        got = grads(ref.pose_to_matrix, torch.float32)
        want = grads(pu.pose_to_matrix, torch.float64)
        same = grads(lambda *a: pu.pose_to_matrix(*a, dtype=torch.float32), torch.float32)
        s = c['s'].double()
        grow = max(1.0, float((1 / s).max())) ** 2 * (max(1.0, float(c['z0'].double().exp().max())) if persp else 1.0)
        tol = 2 * 12 * 16 * U * float(g_mat.abs().max()) * forward_scale(c) * grow
        for k, a, w, r in zip(names, got, want, same):
            assert a.dtype == torch.float32 and w.dtype == torch.float64 and r.dtype == torch.float32
            err = float((a.double() - w.double()).abs().max())
            worst = max(worst, err / tol)
            assert err <= tol, (b, persp, flipped, unit, k, err, tol)
            assert float((r.double() - w.double()).abs().max()) <= tol
    print('float32 autograd of the live pose_to_matrix against float64 autograd of the restatement: worst error / bound %.3f' % worst)


class NumpyOneCopyRule:
    """numpy for lib/pose_utils.py:74, written for numpy 1: np.array(x, dtype, copy=False) meant "copy only if needed", which
    numpy 2 spells np.asarray and otherwise refuses.  Everything else is numpy's own."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def array(obj, dtype=None, copy=True):
        return np.array(obj, dtype=dtype) if copy else np.asarray(obj, dtype=dtype)


@needs_reference
def test_restatement_against_the_live_reference_matrix_to_pose(monkeypatch):
    """Matrices from the float64 restatement of pose_to_matrix, rounded to float32; all four extraction branches (asserted).
    z0, t2, s: t3 is a three-term sum of products (A / w) t - 4 roundings each of size u |t3|_1-like terms - then s = 2 f /
    t3.z and t2 = t3 s: |fp32 - fp64| <= 16 u * max(1, sum_i |A_i| |t_i| / w) * max(1, |s|) * max(1, 1 / |t3.z|).
    Quaternions: compared UP TO SIGN (the branch choice of pose_utils.py:77-92 can flip near a tie and the branches differ
    by the sign of q); entries of the float32 world2cam matrix carry 2 u, the pivot is at least 1, so 16 u covers them.
    Round trip: in float64, on the unrounded matrix, to 1e-12; pose_to_matrix (float64) of the reference's float32 pose of
    the float32 matrix returns that matrix within the two bounds above."""
    ref = reference.modules().pose_utils
    monkeypatch.setattr(ref, 'np', NumpyOneCopyRule())
    hit = set()
    for b, persp, flipped in [(b, p, f) for b in (1, 40) for p in (True, False) for f in (False, True)]:
        c = pu.case(b, persp, turns=b > 1)
        m, focal = (t if t is None else t.float() for t in pu.pose_to_matrix(c['z0'], c['t2'], c['s'], c['q'], flipped))
        z0, t2, s, q = ref.matrix_to_pose(m, focal, flipped)
        cond = ref.matrix_to_conditioning_vector(m, focal, flipped)
        z64, t64, s64, q64, cond64, branches = pu.matrix_to_pose(m, focal, flipped)
        z32, t32, s32, q32, cond32, _ = pu.matrix_to_pose(m, focal, flipped, dtype=torch.float32)
        hit |= set(branches)
        w = pu.world2cam(m.double(), flipped)
        t3 = -w[:, :3, 3]
        sums = float(((m[:, :3, :3].double() / m[:, 3:4, 3:4].double()).abs() * m[:, :3, 3:4].double().abs()).sum(1).max())
        tol = 16 * U * max(1.0, sums) * max(1.0, float(s64.abs().max())) * max(1.0, float((1 / t3[:, 2].abs()).max()) if persp else 1.0)
        assert (z0 is None) == (not persp) and (z64 is None) == (not persp)
        if persp:
            assert float((z0.double() - z64).abs().max()) <= 8 * U * max(1.0, float(z64.abs().max())) and torch.equal(z32, z0)
        for name, a, w64, r32 in (('t2', t2, t64, t32), ('s', s, s64, s32), ('cond', cond, cond64, cond32)):
            assert a.shape == w64.shape and float((a.double() - w64).abs().max()) <= tol, (name, b, persp, flipped)
            assert torch.equal(r32, a), name
        sign = torch.sign((q.double() * q64).sum(-1, keepdim=True))
        assert float((q.double() * sign - q64).abs().max()) <= 16 * U
        assert torch.equal(q32 * torch.sign((q32 * q).sum(-1, keepdim=True)), q)
        # a quaternion that is unit in float64, a matrix that is not rounded to float32: the round trip is then exact
        exact, exact_focal = pu.pose_to_matrix(c['z0'], c['t2'], c['s'], pu.normalize(c['q'].double()), flipped)
        back64, _ = pu.pose_to_matrix(*pu.matrix_to_pose(exact, exact_focal, flipped)[:4], flipped)
        assert float((back64 - exact).abs().max()) <= 1e-12 * forward_scale(c)
        back, _ = pu.pose_to_matrix(z0, t2, s, q, flipped)
        assert float((back - m.double()).abs().max()) <= (16 * U + tol) * forward_scale(c)
    assert hit == {0, 1, 2, 3}, hit


@needs_reference
def test_restatement_against_the_live_reference_distance_and_selection():
    """rotation_matrix_distance at float32 is the reference bit for bit (3 x 3 and 4 x 4 with a non-unit [3,3]); in float64 it
    differs by acos' conditioning: d(acos) = d(c) / sin(angle), d(c) <= 12 u, so between 5 and 175 degrees
    |fp32 - fp64| <= (12 u / sin(5 deg) + 4 u pi) * 180 / pi degrees.  perturb_poses picks the restatement's float32 indices."""
    ref = reference.modules().pose_utils
    g = torch.Generator().manual_seed(5)
    p3, q3 = pu.rotations(64, g), pu.rotations(64, g)
    p4, q4 = pu.poses_4x4(64, 1), pu.poses_4x4(64, 2)
    tol = (12 * U / np.sin(np.radians(5.0)) + 4 * U * np.pi) * 180 / np.pi
    for p, q in ((p3, q3), (p4, q4)):
        d, d64 = ref.rotation_matrix_distance(p, q), pu.rotation_distance(p, q)
        assert torch.equal(pu.rotation_distance(p, q, torch.float32), d)
        inside = (d64 >= 5) & (d64 <= 175)
        assert int(inside.sum()) > 32 and float((d.double() - d64)[inside].abs().max()) <= tol
    for n in (1, 2, 65):
        poses, extra = pu.poses_4x4(n, 3), torch.arange(n)
        out, none, picked = ref.perturb_poses(poses, 15.0, None, extra)
        g = torch.Generator().manual_seed(1234)
        target = torch.cat([torch.rand((1,), generator=g) * 15.0 * 2 for _ in range(n)])
        assert none is None and torch.equal(picked, pu.nearest_by_angle(poses, target, torch.float32)) and torch.equal(out, poses[picked])
