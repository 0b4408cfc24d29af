"""nerf_from_image_amd.pose_utils (csrc/nfi_pose.inc) on the GPU against the float64 restatement of lib/pose_utils.py in
tests/pose_util.py (pinned to the live reference, bit for bit at float32, by tests/test_pose_utils_abi.py).

Sizes of the per-image kernels: B = 1, 3, 64, 65 and 257 - one image, a partial wave, a full wave, one past it, past 256
threads.  The kernels can go wrong at the tail guard, at the branch selection and at the optional pointers only.

Bounds are computed on the CPU, here, never taken from a run of a kernel: max(2 x the float32 reference's own worst distance
to float64 over this file's cases, 4 x 2^-23 x the largest |entry|) - the rule of tests/test_ssim_gpu.py; the factor 2 is for
FMA contraction and summation order.  "The float32 reference" is the restatement run at float32 (the reference's files are
not on the GPU machine; on the CPU the two are the same bits)."""
import functools
import types

import pytest
import torch

import pose_util as pu

SIZES = [1, 3, 64, 65, 257]
FLOOR = 4 * pu.EPS32
# (label, unit quaternions, normalize)
Q_MODES = [('unit', True, False), ('non-unit', False, False), ('non-unit normalised', False, True)]
BRANCHES = [(persp, flipped) for persp in (True, False) for flipped in (False, True)]


def cotangent(b, seed=0):
    g = torch.Generator().manual_seed(77 + seed + b)
    return torch.randn(b, 4, 4, generator=g), torch.randn(b, generator=g)


def reference_gradients(c, flipped, normalize, dtype):
    """Gradients of <cotangent, (mat, focal)> w.r.t. (q, t2, s[, z0]) by autograd of the restatement in `dtype`."""
    persp = c['z0'] is not None
    names = ['q', 't2', 's'] + (['z0'] if persp else [])
    leaves = {k: c[k].clone().to(dtype).requires_grad_() for k in names}
    g_mat, g_focal = cotangent(len(c['s']))
    mat, focal = pu.pose_to_matrix(leaves.get('z0'), leaves['t2'], leaves['s'], leaves['q'], flipped, normalize, dtype=dtype)
    loss = (mat * g_mat.to(dtype)).sum() + ((focal * g_focal.to(dtype)).sum() if persp else 0)
    return dict(zip(names, torch.autograd.grad(loss, [leaves[k] for k in names])))


@functools.lru_cache(maxsize=None)
def pose_bounds():
    """(forward bound, backward bound, forward yardstick, backward yardstick) over every pose_to_matrix case of this file."""
    fwd = bwd = big_f = big_b = 0.0
    for b in SIZES:
        for persp, flipped in BRANCHES:
            for _, unit, normalize in Q_MODES:
                c = pu.case(b, persp, unit)
                args = (c['z0'], c['t2'], c['s'], c['q'], flipped, normalize)
                m64, f64 = pu.pose_to_matrix(*args)
                m32, f32 = pu.pose_to_matrix(*args, dtype=torch.float32)
                fwd = max(fwd, float((m32.double() - m64).abs().max()), float((f32.double() - f64).abs().max()) if persp else 0.0)
                big_f = max(big_f, float(m64.abs().max()), float(f64.abs().max()) if persp else 0.0)
                g64, g32 = reference_gradients(c, flipped, normalize, torch.float64), reference_gradients(c, flipped, normalize, torch.float32)
                bwd = max([bwd] + [float((g32[k].double() - g64[k]).abs().max()) for k in g64])
                big_b = max([big_b] + [float(g64[k].abs().max()) for k in g64])
    return max(2 * fwd, FLOOR * big_f), max(2 * bwd, FLOOR * big_b), fwd, bwd


def to_dev(c, dev, strided=False):
    return {k: None if v is None else (pu.strided(v.to(dev)) if strided else v.to(dev)) for k, v in c.items()}


@pytest.mark.gpu
@pytest.mark.parametrize('B', SIZES)
def test_pose_to_matrix_forward(gpu_device, B):
    """Both branches, both flips, unit q, non-unit q as it is (the formulas are polynomial in q) and normalised in the launch;
    dense and non-contiguous inputs give the same bits; focal is None in the orthographic branch."""
    from nerf_from_image_amd import pose_utils
    tol, _, yard, _ = pose_bounds()
    worst = 0.0
    for persp, flipped in BRANCHES:
        for label, unit, normalize in Q_MODES:
            c = pu.case(B, persp, unit)
            m64, f64 = pu.pose_to_matrix(c['z0'], c['t2'], c['s'], c['q'], flipped, normalize)
            d = to_dev(c, gpu_device)
            kw = dict(normalize=True) if normalize else {}
            mat, focal = pose_utils.pose_to_matrix(d['z0'], d['t2'], d['s'], d['q'], flipped, **kw)
            assert mat.shape == (B, 4, 4) and mat.dtype == torch.float32 and mat.device == d['q'].device and mat.is_contiguous()
            err = float((mat.cpu().double() - m64).abs().max())
            if persp:
                assert focal.shape == (B,) and focal.dtype == torch.float32
                err = max(err, float((focal.cpu().double() - f64).abs().max()))
            else:
                assert focal is None
            worst = max(worst, err)
            assert err <= tol, (persp, flipped, label, err, tol)
            v = to_dev(c, gpu_device, strided=True)
            mat2, focal2 = pose_utils.pose_to_matrix(v['z0'], v['t2'], v['s'], v['q'], camera_flipped=flipped, **kw)
            assert torch.equal(mat2, mat) and (focal2 is None if focal is None else torch.equal(focal2, focal))
            if normalize:       # the fused normalisation against F.normalize outside, as run.py:2257-2262 calls it
                outside, _ = pose_utils.pose_to_matrix(d['z0'], d['t2'], d['s'], torch.nn.functional.normalize(d['q'], dim=-1), flipped)
                assert float((outside - mat).abs().max()) <= tol
    print('pose_to_matrix forward B = %d: worst %.3e (float32 reference %.3e, bound %.3e)' % (B, worst, yard, tol))


@pytest.mark.gpu
@pytest.mark.parametrize('B', SIZES)
def test_pose_to_matrix_backward(gpu_device, B):
    """Gradients of a random cotangent on (mat, focal) against float64 autograd of the restatement; the node is one autograd
    node; a second launch on the same inputs gives the same bits; inputs without requires_grad get None."""
    from nerf_from_image_amd import pose_utils
    from nerf_from_image_amd.autograd import PoseToMatrix
    _, tol, _, yard = pose_bounds()
    worst = 0.0
    g_mat, g_focal = (t.to(gpu_device) for t in cotangent(B))
    for persp, flipped in BRANCHES:
        for label, unit, normalize in Q_MODES:
            c = pu.case(B, persp, unit)
            want = reference_gradients(c, flipped, normalize, torch.float64)
            names = list(want)

            def run(strided=False, only=None):
                d = to_dev(c, gpu_device, strided)
                for k in names:
                    if only is None or k in only:
                        d[k].requires_grad_()
                mat, focal = pose_utils.pose_to_matrix(d['z0'], d['t2'], d['s'], d['q'], flipped, normalize=normalize)
                assert isinstance(mat.grad_fn, PoseToMatrix._backward_cls) and (focal is None) == (not persp)
                loss = (mat * g_mat).sum() + ((focal * g_focal).sum() if persp else 0)
                loss.backward()
                return {k: d[k].grad for k in names}
            got, again, views = run(), run(), run(strided=True)
            for k in names:
                assert got[k].shape == c[k].shape and got[k].dtype == torch.float32
                err = float((got[k].cpu().double() - want[k]).abs().max())
                worst = max(worst, err)
                assert err <= tol, (persp, flipped, label, k, err, tol)
                assert torch.equal(got[k], again[k]) and torch.equal(got[k], views[k]), k
            for only in (('q',), ('t2', 's'), (names[-1],)):
                some = run(only=only)
                for k in names:
                    assert (some[k] is None) if k not in only else torch.equal(some[k], got[k]), (only, k)
    print('pose_to_matrix backward B = %d: worst %.3e (float32 autograd of the reference %.3e, bound %.3e)' % (B, worst, yard, tol))


@pytest.mark.gpu
def test_only_focal_used_and_no_grad_mode(gpu_device):
    """A loss on focal alone reaches z0 only (the other gradients are exact zeros); under no_grad, or with no input that
    requires a gradient, no node is recorded."""
    from nerf_from_image_amd import pose_utils
    d = to_dev(pu.case(3, True), gpu_device)
    for k in d:
        d[k].requires_grad_()
    mat, focal = pose_utils.pose_to_matrix(d['z0'], d['t2'], d['s'], d['q'], True)
    focal.sum().backward()
    assert float((d['z0'].grad.cpu().double() - d['z0'].detach().cpu().double().exp() / 2).abs().max()) <= pose_bounds()[1]
    assert all(float(d[k].grad.abs().max()) == 0.0 for k in ('q', 't2', 's'))
    with torch.no_grad():
        m2, f2 = pose_utils.pose_to_matrix(d['z0'], d['t2'], d['s'], d['q'], True)
    m3, f3 = pose_utils.pose_to_matrix(*(d[k].detach() for k in ('z0', 't2', 's', 'q')), True)
    assert m2.grad_fn is None and m3.grad_fn is None and torch.equal(m2, mat) and torch.equal(m3, mat) and torch.equal(f3, focal)


@pytest.mark.gpu
def test_pose_gradients_through_a_small_render(gpu_device):
    """matrix_to_pose -> pose_to_matrix(normalize=True) -> a 4 x 4 pixel differentiable render: the loss's gradient arrives at
    every pose parameter, finite and not zero."""
    from stand_in import StandInGenerator, look_at_cameras
    import nerf_from_image_amd.generator as nfi_gen
    import nerf_from_image_amd.render as nfi_render
    from nerf_from_image_amd import pose_utils
    torch.manual_seed(4)
    model = StandInGenerator(0.55, attention_values=10, use_sdf=True, plane_res=16).to(gpu_device).eval()
    nfi_gen.attach(model)
    g = torch.Generator().manual_seed(9)
    cam = look_at_cameras(2, 1.6, g).to(gpu_device)
    focal = torch.full((2,), 1.0254, device=gpu_device)
    z = torch.randn(2, 512, generator=g).to(gpu_device)
    params = [t.clone().requires_grad_() for t in pose_utils.matrix_to_pose(cam, focal, False)]
    z0, t2, s, q = params
    cam2, focal2 = pose_utils.pose_to_matrix(z0, t2, s, q * 1.5, False, normalize=True)
    assert float((cam2.detach() - cam).abs().max()) <= 1e-5 and float((focal2.detach() - focal).abs().max()) <= 1e-6
    cfg = types.SimpleNamespace(use_viewdir=False, use_sdf=True, attention_values=10, fine_sampling=True)
    render = nfi_render.make_render(cfg, {'scene_range': 0.55, 'white_background': False})
    rgb, depth, mask, _, _, _ = render(model, 4, 4, cam2, focal2, None, None, z, 16)
    (rgb.sum() + mask.sum()).backward()
    for name, p in zip(('z0', 't2', 's', 'q'), params):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0, name


def matrices(b, persp, flipped):
    """cam2world [b,4,4] and focal [b] or None, float32, from the float64 restatement on quaternions that are unit in float64;
    the first rows turn by 125, 150 and 179 degrees about the axes and near them."""
    c = pu.case(b, persp, turns=True)
    m, f = pu.pose_to_matrix(c['z0'], c['t2'], c['s'], pu.normalize(c['q'].double()), flipped)
    return m.float(), None if f is None else f.float(), c


@functools.lru_cache(maxsize=None)
def inverse_bounds():
    """Per output of matrix_to_pose, the rule of the module docstring over this file's matrix_to_pose cases (quaternions
    up to sign)."""
    names = ('z0', 't2', 's', 'q', 'cond')
    yard, big = dict.fromkeys(names, 0.0), dict.fromkeys(names, 0.0)
    for b in SIZES:
        for persp, flipped in BRANCHES:
            m, f, _ = matrices(b, persp, flipped)
            r64, r32 = pu.matrix_to_pose(m, f, flipped), pu.matrix_to_pose(m, f, flipped, dtype=torch.float32)
            for k, a64, a32 in zip(names, r64, r32):
                if a64 is None:
                    continue
                if k == 'q':
                    a32 = a32 * torch.sign((a32.double() * a64).sum(-1, keepdim=True))
                yard[k] = max(yard[k], float((a32.double() - a64).abs().max()))
                big[k] = max(big[k], float(a64.abs().max()))
    return {k: max(2 * yard[k], FLOOR * big[k]) for k in names}, yard


@pytest.mark.gpu
@pytest.mark.parametrize('B', SIZES)
def test_matrix_to_pose(gpu_device, B):
    """Both branches and flips, all four branches of the quaternion extraction (asserted here, on the CPU); outputs are device
    tensors and the call makes no host transfer (sync debug mode 'error'); quaternions match up to sign, pose_to_matrix of
    the result returns the matrix; the conditioning vector matches the restatement."""
    from nerf_from_image_amd import pose_utils
    tol, yard = inverse_bounds()
    fwd_tol = pose_bounds()[0]
    hit, worst = set(), dict.fromkeys(tol, 0.0)
    for persp, flipped in BRANCHES:
        m, f, c = matrices(B, persp, flipped)
        want = dict(zip(('z0', 't2', 's', 'q', 'cond', 'branches'), pu.matrix_to_pose(m, f, flipped)))
        hit |= set(want['branches'])
        md, fd = m.to(gpu_device), None if f is None else f.to(gpu_device)
        torch.cuda.synchronize(gpu_device)
        torch.cuda.set_sync_debug_mode('error')
        try:
            z0, t2, s, q = pose_utils.matrix_to_pose(md, fd, flipped)
            cond = pose_utils.matrix_to_conditioning_vector(md, fd, flipped)
            strided = pose_utils.matrix_to_pose(pu.strided(md), pu.strided(fd), camera_flipped=flipped)
        finally:
            torch.cuda.set_sync_debug_mode('default')
        got = dict(z0=z0, t2=t2, s=s, q=q, cond=cond)
        assert (z0 is None) == (not persp) and cond.shape == (B, 13)
        for k, a in got.items():
            if a is None:
                continue
            assert a.is_cuda and a.dtype == torch.float32 and a.shape == want[k].shape, k
            a = a.cpu().double()
            if k == 'q':
                a = a * torch.sign((a * want['q']).sum(-1, keepdim=True))
            err = float((a - want[k]).abs().max())
            worst[k] = max(worst[k], err)
            assert err <= tol[k], (k, persp, flipped, err, tol[k])
        for a, b in zip(strided, (z0, t2, s, q)):
            assert (a is None and b is None) or torch.equal(a, b)
        back, back_focal = pose_utils.pose_to_matrix(z0, t2, s, q, flipped)
        # the matrix is a float32 rounding of a similarity matrix: the pose read from it is off by the inverse bounds, which the
        # forward map scales by no more than its largest entry
        scale = max(1.0, float(m.abs().max()))
        assert float((back.cpu().double() - m.double()).abs().max()) <= fwd_tol + scale * (tol['q'] * 4 + tol['t2'] + tol['s'])
        if persp:
            assert float((back_focal.cpu() - f).abs().max()) <= fwd_tol + float(f.max()) * tol['z0']
    if B >= 27:
        assert hit == {0, 1, 2, 3}, hit
    print('matrix_to_pose B = %d: worst %s; float32 reference %s' % (
        B, ', '.join('%s %.2e' % kv for kv in worst.items()), ', '.join('%s %.2e' % kv for kv in yard.items())))


def test_the_turns_take_every_extraction_branch():
    """CPU: the cases of test_matrix_to_pose with at least 27 rows reach all four branches of pose_utils.py:77-92."""
    for b in (64, 65, 257):
        for persp, flipped in BRANCHES:
            m, f, _ = matrices(b, persp, flipped)
            assert set(pu.matrix_to_pose(m, f, flipped)[5]) == {0, 1, 2, 3}


def turned(p, degrees, g):
    """p [n,3,3] times a turn by degrees [n] about a random axis, float32."""
    axis = torch.randn(len(p), 3, generator=g).double()
    axis = axis / axis.norm(dim=-1, keepdim=True)
    half = torch.deg2rad(degrees.double()) / 2
    q = torch.cat([half.cos()[:, None], axis * half.sin()[:, None]], dim=1)
    return (p.double() @ pu.rotation_rows(q)).float()


def as_4x4(r, g):
    """[[h r, t], [0, h]] with h in [0.5, 2]: the 4 x 4 form divides by h again."""
    h = 0.5 + 1.5 * torch.rand(len(r), generator=g)
    m = torch.zeros(len(r), 4, 4)
    m[:, :3, :3], m[:, :3, 3], m[:, 3, 3] = r * h[:, None, None], torch.randn(len(r), 3, generator=g), h
    return m


@pytest.mark.gpu
@pytest.mark.parametrize('B', SIZES)
def test_rotation_matrix_distance(gpu_device, B):
    """3 x 3 and 4 x 4 (non-unit [3,3]) pairs.  Angles in [5, 175] degrees: the rule of the module docstring, in degrees.
    Identical and opposite rotations, where acos is ill-conditioned: finite, inside [0, 180], and no further from float64 than
    twice the float32 reference's own worst error on the same pairs."""
    from nerf_from_image_amd import pose_utils
    g = torch.Generator().manual_seed(11 + B)
    p = pu.rotations(B, g)
    angles = 5 + 170 * torch.rand(B, generator=g)
    sets = {'inside': turned(p, angles, g), 'identical': p.clone(), 'opposite': turned(p, torch.full((B,), 180.0), g)}
    for dim in (3, 4):
        for name, q in sets.items():
            a, b = (p, q) if dim == 3 else (as_4x4(p, g), as_4x4(q, g))
            d64, d32 = pu.rotation_distance(a, b), pu.rotation_distance(a, b, torch.float32)
            yard = float((d32.double() - d64).abs().max())
            got = pose_utils.rotation_matrix_distance(a.to(gpu_device), b.to(gpu_device))
            assert got.shape == (B,) and got.dtype == torch.float32 and got.is_cuda
            assert torch.equal(pose_utils.rotation_matrix_distance(pu.strided(a.to(gpu_device)), pu.strided(b.to(gpu_device))), got)
            got = got.cpu().double()
            err = float((got - d64).abs().max())
            if name == 'inside':
                assert float(d64.min()) > 4.9 and float(d64.max()) < 175.1
                tol = max(2 * yard, FLOOR * float(d64.max()))
            else:
                assert bool(torch.isfinite(got).all()) and float(got.min()) >= 0.0 and float(got.max()) <= 180.0
                # (one float32 spacing at the largest value: what a float32 result must be allowed in any case)
                tol = max(2 * yard, pu.EPS32 * float(d64.max()))
            print('rotation_matrix_distance B = %d, %d x %d, %s: %.3e (float32 reference %.3e, bound %.3e)' % (B, dim, dim, name, err, yard, tol))
            assert err <= tol, (dim, name, err, tol)


@pytest.mark.gpu
@pytest.mark.parametrize('N', [1, 2, 65, 300])
def test_perturb_poses(gpu_device, N):
    from nerf_from_image_amd import pose_utils
    poses = pu.poses_4x4(N, 7)
    dev_poses = poses.to(gpu_device)
    rows = torch.arange(N, device=gpu_device)
    focal = torch.rand(N, generator=torch.Generator().manual_seed(N)).to(gpu_device)
    bbox = torch.rand(N, 4, generator=torch.Generator().manual_seed(N + 1))          # an extra argument on the host
    out, picked, none, f, bb = pose_utils.perturb_poses(dev_poses, 15.0, rows, None, focal, bbox)
    # (c) gathered and cloned as the reference does, a None stays None
    assert none is None and picked.shape == (N,) and out.shape == (N, 4, 4)
    assert torch.equal(out, dev_poses[picked]) and torch.equal(f, focal[picked]) and torch.equal(bb, bbox[picked.cpu()]) and picked.dtype == torch.int64
    assert out.data_ptr() != dev_poses.data_ptr() and f.data_ptr() != focal.data_ptr() and out.is_contiguous()
    # (d) the same on two calls
    again = pose_utils.perturb_poses(dev_poses, 15.0, rows)
    assert torch.equal(again[1], picked) and torch.equal(again[0], out)
    # (a) optimal within tolerance, measured with float64 distances
    target = pose_utils.perturb_targets(N, 15.0)
    gap = (pu.pairwise_distance(poses) - target.double()[:, None]).abs()
    best = gap.min(dim=1).values
    ours = gap[torch.arange(N), picked.cpu().long()] - best
    theirs = gap[torch.arange(N), pu.nearest_by_angle(poses, target, torch.float32)] - best
    tol = max(2 * float(theirs.max()), 1e-4)
    print('perturb_poses N = %d: sub-optimality %.3e degrees (float32 reference %.3e, bound %.3e)' % (N, float(ours.max()), float(theirs.max()), tol))
    assert float(ours.max()) <= tol
    # (b) the tie rule: N copies of one matrix
    same = dev_poses[:1].expand(N, 4, 4).contiguous()
    assert pose_utils.perturb_poses(same, 15.0, rows)[1].tolist() == [0] * N


@pytest.mark.gpu
@pytest.mark.parametrize('B', SIZES)
def test_project_pose(gpu_device, B):
    """In place, on parameters too; equal to run.py:2307-2310: |s| and the clamp exactly, the normalisation within 4 x 2^-23
    (entries are at most 1; F.normalize rounds four times - squares' sum, root, quotient - and the kernel once); a zero
    quaternion stays zero (F.normalize's eps), z0=None is accepted."""
    from nerf_from_image_amd import pose_utils
    g = torch.Generator().manual_seed(B)
    q = pu.random_quaternions(B, g, unit=False)
    q[B // 2] = 0.0
    s = torch.randn(B, generator=g)
    z0 = torch.randn(B, generator=g) * 4
    z0[0], s[0] = 7.0, -0.0
    want_q, want_s, want_z0 = pu.project(q, s, z0)
    for with_z0 in (True, False):
        dq, ds, dz = (torch.nn.Parameter(t.clone().to(gpu_device)) for t in (q, s, z0))
        ptrs = [t.data_ptr() for t in (dq, ds, dz)]
        assert pose_utils.project_pose_(dq, ds, dz if with_z0 else None) is None
        assert [t.data_ptr() for t in (dq, ds, dz)] == ptrs and dq.requires_grad and dq.is_leaf
        assert bool(torch.isfinite(dq).all()) and float(dq[B // 2].abs().max()) == 0.0
        assert float((dq.detach().cpu() - want_q).abs().max()) <= FLOOR
        assert torch.equal(ds.detach().cpu(), want_s) and not bool(torch.signbit(ds.detach().cpu()).any())
        assert torch.equal(dz.detach().cpu(), want_z0 if with_z0 else z0)
    with pytest.raises(ValueError, match='contiguous'):
        pose_utils.project_pose_(pu.strided(q.to(gpu_device)), s.to(gpu_device))


@pytest.mark.gpu
def test_capture_and_replay(gpu_device):
    """pose_to_matrix(normalize=True) then project_pose_ captured in one graph on one stream (no branches); two replays with new
    parameter values copied in equal the eager results bit for bit."""
    from nerf_from_image_amd import pose_utils
    B = 5
    values = [to_dev(pu.case(B, True, unit=False, seed=k), gpu_device) for k in (1, 2, 3)]
    static = {k: v.clone() for k, v in values[0].items()}

    def step(p):
        mat, focal = pose_utils.pose_to_matrix(p['z0'], p['t2'], p['s'], p['q'], True, normalize=True)
        pose_utils.project_pose_(p['q'], p['s'], p['z0'])
        return mat, focal
    step({k: v.clone() for k, v in values[0].items()})          # the kernels are loaded before the capture
    torch.cuda.synchronize(gpu_device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mat, focal = step(static)
    for new in values[1:]:
        for k in static:
            static[k].copy_(new[k])
        graph.replay()
        torch.cuda.synchronize(gpu_device)
        eager = {k: v.clone() for k, v in new.items()}
        want_mat, want_focal = step(eager)
        assert torch.equal(mat, want_mat) and torch.equal(focal, want_focal)
        for k in static:
            assert torch.equal(static[k], eager[k]), k
        assert not torch.equal(static['q'], new['q'])
