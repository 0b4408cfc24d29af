"""The per-ray trunk of ViewDirectionMapper (models/generator.py:194-241) as HIP kernels: nfi_viewdir_mapper_fwd / _bwd,
ops.viewdir_mapper_fwd / _bwd, generator.hip_ray_feature and attach(..., hip_viewdir_mapper=True).

Comparator: the reference's own class with seeded, non-zero weights in every layer (biases and norm affines included), a
float64 deep copy as the truth and the fp32 original, on the same device and inputs, as the yardstick.  Distance of a
tensor: max|a - truth| / max|truth|.  Bound: the HIP result is at most RATIO x as far from the truth as the fp32 reference
is, the reference's distance taken as at least FLOOR = 64 * 2^-24 (the worst-case rounding of one 64-term fp32 dot
product; it keeps a reference that happens to hit the truth from being a zero denominator).  Every test prints both
distances per tensor."""
import copy
import ctypes
import re

import pytest
import torch

import nerf_from_image_amd.generator as nfi_gen
from nerf_from_image_amd import _lib, ops
from oracle import reference

RATIO, FLOOR = 2.5, 64 * 2.0 ** -24
PTR = 16
PARAM_NAMES = [n for n, _ in ops.VIEWDIR_MAPPER_PARAMS]


# ------------------------------------------------------------------------------------------------------------------
# without a GPU: header, exports, argument rules
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    return _lib.load()


def _placeholder_args(**kw):
    fields = {n: PTR for n, t in _lib.STRUCT_FIELDS['nfi_viewdir_mapper_args'] if t is ctypes.c_void_p}
    fields['n_rays'] = 100
    fields.update(kw)
    return _lib.make_args('nfi_viewdir_mapper_args', **fields)


def test_header_declares_the_mapper_entries():
    src = open(_lib.HEADER).read()
    declared = set(re.findall(r'\b(nfi_[a-z_0-9]+)\s*\(', src))
    assert {'nfi_viewdir_mapper_fwd', 'nfi_viewdir_mapper_bwd'} <= declared
    assert {'nfi_viewdir_mapper_fwd', 'nfi_viewdir_mapper_bwd'} <= set(_lib.FUNCTIONS)
    f = [n for n, _ in _lib.STRUCT_FIELDS['nfi_viewdir_mapper_args']]
    assert f[:2] == ['n_rays', 'viewdir'] and f[2:20] == PARAM_NAMES and f[20:22] == ['feature', 'g_feature']
    assert f[22:40] == ['g_' + n for n in PARAM_NAMES] and f[40:] == ['g_viewdir']
    assert 'models/generator.py:194-241' in src          # the entry cites the reference lines it replaces


def test_library_exports_the_mapper_entries(lib):
    for name in ('nfi_viewdir_mapper_fwd', 'nfi_viewdir_mapper_bwd'):
        assert hasattr(lib, name), name


@pytest.mark.parametrize('entry', ['nfi_viewdir_mapper_fwd', 'nfi_viewdir_mapper_bwd'])
def test_bad_mapper_arguments_are_rejected_before_any_launch(lib, entry):
    fn = getattr(lib, entry)
    assert fn(None, None) == -1 and b'null' in lib.nfi_last_error()
    for field in ('viewdir', 'fc0_w', 'norm3_b', 'fc6_b', 'feature' if entry.endswith('fwd') else 'g_feature'):
        a = _placeholder_args(**{field: None})
        assert fn(ctypes.byref(a), None) == -1 and b'null' in lib.nfi_last_error(), field
    if entry.endswith('bwd'):
        a = _placeholder_args(g_norm2_w=None)          # the 18 parameter gradients: all or none
        assert fn(ctypes.byref(a), None) == -1 and b'all 18 or none' in lib.nfi_last_error()
        a = _placeholder_args(g_viewdir=None, **{'g_' + n: None for n in PARAM_NAMES})
        assert fn(ctypes.byref(a), None) == -1 and b'nothing to compute' in lib.nfi_last_error()
    for n in (0, -5):
        a = _placeholder_args(n_rays=n)
        assert fn(ctypes.byref(a), None) == -1 and b'n_rays' in lib.nfi_last_error(), n


# ------------------------------------------------------------------------------------------------------------------
# on the GPU
# ------------------------------------------------------------------------------------------------------------------
def _require_reference():
    if not reference.available():
        pytest.skip('reference sources not staged: run oracle/make_ref.py (or __graft_entry__.build()) where the reference checkout exists')


_mappers = {}


def mappers(dev):
    """(fp32 reference mapper, its float64 copy), both on dev, built once."""
    if 'm' not in _mappers:
        gen = torch.Generator().manual_seed(4321)
        torch.manual_seed(4321)
        m = reference.modules().generator.ViewDirectionMapper(10, 32)
        with torch.no_grad():
            for name, p in m.named_parameters():
                if name.startswith('norm') and name.endswith('weight'):
                    p.copy_(1.0 + 0.3 * torch.randn(p.shape, generator=gen))
                elif name.endswith('bias'):
                    p.copy_(0.3 * torch.randn(p.shape, generator=gen))
                else:
                    p.copy_(torch.randn(p.shape, generator=gen))
        m = m.to(dev)
        _mappers['m'] = (m, copy.deepcopy(m).double())
    return _mappers['m']


def trunk(m, v):
    """fc6's output of the real class (its forward returns a closure; the hook is what the package itself uses)."""
    with nfi_gen._capture_ray_feature(m) as cap:
        m(v)
    return cap['x']


def directions(n, dev, seed=0):
    """n unit vectors: the six axis directions first, then pairs (d, -d) of exact sign flips, then random ones."""
    gen = torch.Generator().manual_seed(seed + n)
    d = torch.randn(n, 3, generator=gen)
    d = d / d.norm(dim=-1, keepdim=True)
    axes = torch.cat([torch.eye(3), -torch.eye(3)])
    k = min(n, 6)
    d[:k] = axes.roll(-2, 0)[:k]                      # (n = 1: +z)
    for i in range(6, min(n, 26) - 1, 2):
        d[i + 1] = -d[i]
    return d.to(dev)


KINKED = ('fc0', 'norm1', 'norm2', 'norm3', 'norm4', 'fc5')       # the layers a LeakyReLU follows


def clear_of_kinks(d, m64, seed):
    """The backward cases' directions, with every ray replaced (by a fresh seeded unit vector) that puts a LeakyReLU's
    input within fp32 rounding of zero.  The slope jumps from 0.2 to 1 there, so the gradient of such a ray is decided by
    the last bit of the forward: any two fp32 evaluations - the reference's own on another device included - may
    legitimately land on different sides, and a distance from float64 says nothing.  'Within rounding': |input| below
    FLOOR (one 64-term fp32 dot product) x the layer's largest input, measured on the float64 module.  (First seen at
    N = 3219: norm2's output of one ray 2.5e-8 from zero.)  The forward cases keep every ray: the activation itself is
    continuous.

    How many to expect: a ray has 6 x 64 such inputs, of magnitude ~1 with a density of ~0.4 around zero, and the window is
    2 x FLOOR x (the layer's largest input, 3 ... 5): 384 x 0.4 x 2 x 3.8e-6 x 4 = 0.5 % of the rays (seen: 14 of 3219, 36
    of 8197).  The count is printed and asserted to stay below 1 % of N (+ 1): a module or a rule that throws out more is
    a finding, not an input selection.  Among the replaced may be one of the 26 named directions (axes, sign flips) at the
    head - printed too; the forward cases check those on every N."""
    gen = torch.Generator().manual_seed(seed)
    d0, n = d, d.shape[0]
    for _ in range(20):
        pre = {}
        hooks = [getattr(m64, k).register_forward_hook(lambda mod, i, o, k=k: pre.__setitem__(k, o.detach().clone())) for k in KINKED]
        with torch.no_grad():
            m64(d.double().unsqueeze(-2))
        for h in hooks:
            h.remove()
        bad = torch.zeros(d.shape[0], dtype=torch.bool, device=d.device)
        for k in KINKED:
            a = pre[k].abs().view(d.shape[0], -1)
            bad |= (a < FLOOR * a.max()).any(dim=1)
        if not bad.any():
            moved = (d != d0).any(dim=1)
            print('clear_of_kinks: N = %d, %d rays replaced (%d of the 26 named directions)' % (n, int(moved.sum()), int(moved[:26].sum())))
            assert int(moved.sum()) <= 0.01 * n + 1, (int(moved.sum()), n)
            return d
        fresh = torch.randn(int(bad.sum()), 3, generator=gen)
        d = d.clone()
        d[bad] = (fresh / fresh.norm(dim=-1, keepdim=True)).to(d.device)
    raise AssertionError('no kink-free directions found')


def dist(a, truth):
    return float((a.double() - truth).abs().max() / truth.abs().max())


def check(name, ours, ref32, truth):
    d_hip, d_ref = dist(ours, truth), dist(ref32, truth)
    print('%-12s |truth|max %.3e   HIP %.3e   fp32 reference %.3e   ratio %.2f' % (
        name, float(truth.abs().max()), d_hip, d_ref, d_hip / max(d_ref, FLOOR)))
    return None if d_hip <= RATIO * max(d_ref, FLOOR) else (name, d_hip, d_ref)


def params_of(m):
    return [p.detach() for p in nfi_gen.viewdir_mapper_parameters(m)]


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 15, 16, 17, 63, 64, 65, 126, 256, 3219, 8197])
def test_forward(gpu_device, n):
    _require_reference()
    m32, m64 = mappers(gpu_device)
    v = directions(n, gpu_device).view(n, 1, 3)
    with torch.no_grad():
        truth, ref32 = trunk(m64, v.double()), trunk(m32, v.clone())
        ours = ops.viewdir_mapper_fwd(v, params_of(m32))
    assert ours.shape == ref32.shape == (n, 1, 32)
    assert check('feature', ours, ref32, truth) is None


@pytest.mark.gpu
@pytest.mark.parametrize('norm', [1e-3, 30.0])
def test_forward_of_unnormalised_directions(gpu_device, norm):
    """LayerNorm makes the trunk robust to the scale of its input; fc0 (bias, activation) in front of it is not."""
    _require_reference()
    m32, m64 = mappers(gpu_device)
    v = (directions(257, gpu_device, seed=3) * norm).view(257, 1, 3)
    with torch.no_grad():
        truth, ref32 = trunk(m64, v.double()), trunk(m32, v.clone())
        ours = ops.viewdir_mapper_fwd(v, params_of(m32))
    assert check('feature', ours, ref32, truth) is None


@pytest.mark.gpu
def test_forward_is_deterministic(gpu_device):
    _require_reference()
    m32, _ = mappers(gpu_device)
    v = directions(8197, gpu_device)
    a = ops.viewdir_mapper_fwd(v, params_of(m32))
    b = ops.viewdir_mapper_fwd(v, params_of(m32))
    assert torch.equal(a, b)


def upstream(n, kind, dev):
    gen = torch.Generator().manual_seed(77 + n)
    g = torch.randn(n, 1, 32, generator=gen)
    if kind == 'half_zero':
        g[torch.rand(n, generator=gen) < 0.5] = 0.0
        g[0] = 0.0
    elif kind == 'magnitudes':
        g = g * 10.0 ** (torch.rand(n, 1, 1, generator=gen) * 9.0 - 6.0)         # per ray: 10^U(-6, 3)
    return g.to(dev)


def reference_gradients(m, v, g):
    """autograd of the real class: (g_viewdir, the 18 parameter gradients in the kernels' order)."""
    m = copy.deepcopy(m).requires_grad_(True)
    v = v.clone().requires_grad_()
    loss = (trunk(m, v) * g).sum()
    grads = torch.autograd.grad(loss, [v] + nfi_gen.viewdir_mapper_parameters(m))
    return grads[0], grads[1:]


_truth_cache = {}


def backward_case(n, kind, dev):
    """(viewdir, upstream, reference fp32 gradients, float64 gradients), computed once per case and left unchanged."""
    if (n, kind) not in _truth_cache:
        m32, m64 = mappers(dev)
        v, g = clear_of_kinks(directions(n, dev), m64, n).view(n, 1, 3), upstream(n, kind, dev)
        _truth_cache[(n, kind)] = (v, g, reference_gradients(m32, v, g), reference_gradients(m64, v.double(), g.double()))
    return _truth_cache[(n, kind)]


def check_gradients(got, ref32, truth, scale=1.0):
    bad = [check('g_viewdir', got['g_viewdir'], ref32[0], truth[0])] if got['g_viewdir'] is not None else []
    for i, name in enumerate(PARAM_NAMES):
        bad.append(check('g_' + name, got['g_' + name], ref32[1][i] * scale, truth[1][i] * scale))
    bad = [b for b in bad if b is not None]
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize('n,kind', [(1, 'random'), (17, 'random'), (65, 'random'), (256, 'random'), (3219, 'random'),
                                    (8197, 'random'), (3219, 'half_zero'), (3219, 'magnitudes')])
def test_backward(gpu_device, n, kind):
    _require_reference()
    m32, _ = mappers(gpu_device)
    v, g, ref32, truth = backward_case(n, kind, gpu_device)
    got = ops.viewdir_mapper_bwd(v, params_of(m32), g)
    assert got['g_viewdir'].shape == v.shape
    check_gradients(got, ref32, truth)


@pytest.mark.gpu
def test_backward_without_the_direction_gradient(gpu_device):
    """g_viewdir = NULL: the parameter gradients alone."""
    _require_reference()
    m32, _ = mappers(gpu_device)
    v, g, ref32, truth = backward_case(3219, 'random', gpu_device)
    got = ops.viewdir_mapper_bwd(v, params_of(m32), g, want_viewdir=False)
    assert got['g_viewdir'] is None
    check_gradients(got, ref32, truth)


@pytest.mark.gpu
def test_backward_accumulates_into_the_callers_buffers(gpu_device):
    """The contract include/nfi_hip.h documents: the parameter gradients are ADDED to what the buffers hold (two calls
    into the same buffers give twice the gradient), g_viewdir is written."""
    _require_reference()
    m32, _ = mappers(gpu_device)
    v, g, ref32, truth = backward_case(8197, 'random', gpu_device)
    first = ops.viewdir_mapper_bwd(v, params_of(m32), g)
    held = {k: t for k, t in first.items()}
    second = ops.viewdir_mapper_bwd(v, params_of(m32), g, into=first)
    for name in PARAM_NAMES:
        assert second['g_' + name] is held['g_' + name]
    assert second['g_viewdir'] is not held['g_viewdir'] and torch.equal(second['g_viewdir'], held['g_viewdir'])
    check_gradients(second, ref32, truth, scale=2.0)


@pytest.mark.gpu
def test_autograd_node(gpu_device):
    """generator.hip_ray_feature: one node, [...,1,32] on viewdir's leading dimensions, gradients to viewdir and the module's
    own parameters; a viewdir without a gradient gets none."""
    _require_reference()
    m32, _ = mappers(gpu_device)
    v, g, ref32, truth = backward_case(3219, 'random', gpu_device)
    m = copy.deepcopy(m32).requires_grad_(True)
    vv = v.view(3, 1073, 1, 3).clone().requires_grad_()
    x = nfi_gen.hip_ray_feature(m, vv)
    assert x.shape == (3, 1073, 1, 32)
    (x * g.view(3, 1073, 1, 32)).sum().backward()
    got = {'g_' + n: p.grad for n, p in zip(PARAM_NAMES, nfi_gen.viewdir_mapper_parameters(m))}
    got['g_viewdir'] = vv.grad.view(-1, 1, 3)
    check_gradients(got, ref32, truth)
    x = nfi_gen.hip_ray_feature(m, v.view(3, 1073, 1, 3))
    seen = {}
    keep = ops.viewdir_mapper_bwd
    ops.viewdir_mapper_bwd = lambda *a, **k: seen.update(k) or keep(*a, **k)
    try:
        x.sum().backward()
    finally:
        ops.viewdir_mapper_bwd = keep
    assert seen == {'want_viewdir': False, 'want_params': True}


@pytest.mark.gpu
def test_frozen_mapper_gets_the_direction_gradient_alone(gpu_device):
    """Parameters without a gradient (the inversion loop): the node asks for g_viewdir only - the entry is called without
    parameter-gradient pointers - and g_viewdir is what the full backward gives; also from an upstream gradient that sits
    at an odd storage offset (the kernel reads it in 16-byte vectors)."""
    _require_reference()
    m32, _ = mappers(gpu_device)
    v, g, ref32, truth = backward_case(3219, 'random', gpu_device)
    vv = v.clone().requires_grad_()
    x = nfi_gen.hip_ray_feature(copy.deepcopy(m32).requires_grad_(False), vv)
    seen = {}
    keep = ops.viewdir_mapper_bwd
    ops.viewdir_mapper_bwd = lambda *a, **k: seen.update(k) or keep(*a, **k)
    try:
        (x * g).sum().backward()
    finally:
        ops.viewdir_mapper_bwd = keep
    assert seen == {'want_viewdir': True, 'want_params': False}
    assert check('g_viewdir', vv.grad, ref32[0], truth[0]) is None
    shifted = torch.cat([g.new_zeros(1), g.flatten()])[1:].view(g.shape)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    got = ops.viewdir_mapper_bwd(v, params_of(m32), shifted, want_params=False)
    assert got['g_fc0_w'] is None and check('g_viewdir', got['g_viewdir'], ref32[0], truth[0]) is None
    with pytest.raises(ValueError):
        ops.viewdir_mapper_bwd(v, params_of(m32), g, want_viewdir=False, want_params=False)


@pytest.mark.gpu
def test_wiring_on_a_bare_container(gpu_device):
    """generator.hip_forward (a container without a forward of its own) with the switch on and off: a stand-in generator
    carrying a mapper of the real shape.  Same sampler outputs, same gradients, the trunk's modules not called."""
    import os
    import sys
    from stand_in import StandInGenerator
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    from viewdir_mapper_bench import Trunk
    torch.manual_seed(3)
    model = StandInGenerator(0.55, use_viewdir=True, plane_res=16)
    model.viewdir_mapper = Trunk()
    model = model.to(gpu_device)
    gen = torch.Generator().manual_seed(8)
    B, H, W, S = 2, 9, 9, 5
    z = torch.randn(B, 512, generator=gen).to(gpu_device)
    x_in = ((torch.rand(B, H, W, S, 3, generator=gen) * 2 - 1) * 0.5).to(gpu_device)
    w_rgb = torch.randn(B, H * W * S, 3, generator=gen).to(gpu_device)
    res = {}
    for on in (False, True):
        m = nfi_gen.attach(copy.deepcopy(model), hip_viewdir_mapper=on)
        calls = []
        h = m.viewdir_mapper.fc1.register_forward_hook(lambda *a: calls.append(1))
        v = directions(B * H * W, gpu_device).view(B, H, W, 1, 3).requires_grad_()
        out = m(v, z, ['sampler'])['sampler'](x_in, ['sigma', 'rgb'])
        h.remove()
        (out['rgb'].reshape(B, -1, 3) * w_rgb).sum().backward()
        res[on] = (len(calls), out['rgb'].detach(), v.grad, m.viewdir_mapper.fc3.weight.grad, m.viewdir_mapper.norm1.bias.grad)
        assert '_nfi_capture' not in m.viewdir_mapper.__dict__
    assert res[False][0] == 1 and res[True][0] == 0
    assert float((res[True][1] - res[False][1]).abs().max()) <= 1e-5
    for name, a, b in zip(('g_viewdir', 'g_fc3_w', 'g_norm1_b'), res[True][2:], res[False][2:]):
        err = float((a - b).norm() / b.norm())
        print('%-10s |off| %.3e   relative L2 of on - off %.3e' % (name, float(b.norm()), err))
        assert float(b.norm()) > 0 and err <= 1e-4, (name, err)


# ---- wiring, on the real carla generator ----
def _wired(sc, on):
    twin = copy.copy(sc)
    twin.hip = nfi_gen.attach(copy.deepcopy(sc.gen), hip_viewdir_mapper=on)
    with torch.no_grad():
        # default-initialised norm affines and biases are ones / zeros: give every layer of the trunk seeded weights
        gen = torch.Generator().manual_seed(99)
        for name, p in twin.hip.viewdir_mapper.named_parameters():
            if name.startswith('output'):
                continue
            if name.startswith('norm') and name.endswith('weight'):
                p.copy_((1.0 + 0.3 * torch.randn(p.shape, generator=gen)).to(p.device))
            elif name.endswith('bias'):
                p.copy_((0.3 * torch.randn(p.shape, generator=gen)).to(p.device))
    twin.hip.viewdir_mapper.requires_grad_(True)
    return twin


WIRED_LEAVES = ('fc0.weight', 'fc3.weight', 'norm2.weight', 'fc6.bias')
# the bounds of test_reference_gpu.py::test_gradients_match_the_real_reference for its carla row (3 x measured + 1e-6, relative
# L2): latents max(3.8e-6, 2.2e-5), camera 3.6e-5; the mapper's parameters sit on the camera gradient's path (the view
# directions) and take its bound
WIRED_BOUND = dict(ws=3.0 * 2.2e-5 + 1e-6, cam=3.0 * 3.6e-5 + 1e-6, mapper=3.0 * 3.6e-5 + 1e-6)


def _wired_run(twin, rc, res, samples, noise, w_rgb, w_mask, hip_options=None, **render_kw):
    counts = {'fc1': 0, 'norm4': 0}
    mp = twin.hip.viewdir_mapper
    hooks = [mp.fc1.register_forward_hook(lambda *a: counts.__setitem__('fc1', counts['fc1'] + 1)),
             mp.norm4.register_forward_hook(lambda *a: counts.__setitem__('norm4', counts['norm4'] + 1))]
    ws, cam = twin.ws.detach().clone().requires_grad_(), twin.cam.detach().clone().requires_grad_()
    twin.hip.zero_grad()
    try:
        out = rc.hip_render(twin, res, samples, noise, grad=True, ws=ws, cam=cam, hip_options=hip_options, **render_kw)
    finally:
        for h in hooks:
            h.remove()
    ((out[0] * w_rgb).sum() + (out[2] * w_mask).sum()).backward()
    named = dict(mp.named_parameters())
    grads = {k: named[k].grad.detach().clone() for k in WIRED_LEAVES}
    grads['ws'], grads['cam'] = ws.grad, cam.grad
    return counts, [o.detach() for o in out[:3]], grads


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['plain', 'two_views', 'no_cam_grad'])
def test_wiring_on_the_real_carla_generator(gpu_device, variant):
    """attach(..., hip_viewdir_mapper=True) against the default on the reference's own Generator (its forward wrapped):
    the trunk's modules are not called, the render and its gradients are those of the PyTorch trunk.

    Measured (MI355X, three sessions): `plain` and `no_cam_grad` every leaf 7e-7 ... 3.4e-6 in all three.  `two_views`: 9e-7
    ... 2.3e-6 in the first session, and in the two after it the four mapper leaves at 3.8e-5 ... 1.111e-4 / 1.110e-4
    (fc6.bias, bound 1.09e-4: a FAILURE by 2 %, the same figure both times).  fc6.bias's gradient is the plain sum of the upstream gradient, which the trunk's backward
    does not touch: the difference is made downstream, where the two fp32 trunks' last bits decide the slope of
    leaky_relu(ray feature + sample feature) for the odd one of the 16.8 M sample features of a render; which sample that
    is moves with the last bits of the planes, i.e. with the convolution solver a session gets.  That reading is an
    inference from which leaf is worst, not a traced sample.  The bounds are the issue's and stay."""
    _require_reference()
    import reference_cases as rc
    res, samples = 64, 32
    with rc.deterministic_producer():
        sc = rc.build_scene('carla', 2, gpu_device)
        off, on = _wired(sc, False), _wired(sc, True)
        hip_options, render_kw = None, {}
        if variant == 'two_views':
            hip_options = {'views_per_scene': 2}
            for t in (off, on):
                t.ws = t.ws[:1]              # one scene, the two cameras are its views
        if variant == 'no_cam_grad':
            render_kw = {'force_no_cam_grad': True}
        noise = rc.draw_noise(sc, res, samples)
        gw = torch.Generator(device=gpu_device).manual_seed(5)
        w_rgb = torch.randn((sc.batch, res, res, 3), device=gpu_device, generator=gw)
        w_mask = torch.randn((sc.batch, res, res), device=gpu_device, generator=gw)
        seen = {}
        keep = ops.viewdir_mapper_bwd
        ops.viewdir_mapper_bwd = lambda *a, **k: seen.update(k) or keep(*a, **k)
        try:
            c_off, o_off, g_off = _wired_run(off, rc, res, samples, noise, w_rgb, w_mask, hip_options, **render_kw)
            c_on, o_on, g_on = _wired_run(on, rc, res, samples, noise, w_rgb, w_mask, hip_options, **render_kw)
        finally:
            ops.viewdir_mapper_bwd = keep
    assert c_off == {'fc1': 1, 'norm4': 1} and c_on == {'fc1': 0, 'norm4': 0}, (c_off, c_on)
    assert seen == {'want_viewdir': variant != 'no_cam_grad', 'want_params': True}, seen
    for k, a, b in zip(('rgb', 'depth', 'mask'), o_on, o_off):
        print('%-6s max |on - off| %.3e' % (k, rc.max_err(a, b)))
        assert rc.max_err(a, b) <= 1e-4, k
    for k in g_off:
        bound = WIRED_BOUND.get(k, WIRED_BOUND['mapper'])
        a, b = (g_on[k][:, :3], g_off[k][:, :3]) if k == 'cam' else (g_on[k], g_off[k])
        err = rc.rel_err(a, b)
        print('%-14s |off| %.3e   relative L2 of on - off %.3e   bound %.1e' % (k, float(b.norm()), err, bound))
        assert float(b.norm()) > 0 and err <= bound, (k, err, bound)


@pytest.mark.gpu
def test_the_closure_of_the_replaced_forward(gpu_device):
    """The mapper instance's new forward returns a closure of the class's meaning: the reference's own sampler code can
    still call it."""
    _require_reference()
    m32, _ = mappers(gpu_device)
    ours = copy.deepcopy(m32)
    with torch.no_grad():
        ours.output.weight.normal_()
        ours.output.bias.normal_()
    theirs = copy.deepcopy(ours)
    import types
    ours.forward = types.MethodType(nfi_gen._hip_mapper_forward, ours)
    v = directions(130, gpu_device).view(2, 5, 13, 1, 3)
    feats = torch.randn(2, 5 * 13 * 7, 32, device=gpu_device)
    with torch.no_grad():
        closure = ours(v)
        a, b = closure(feats), theirs(v)(feats.clone())
    assert closure.ray_feature.shape == (2, 5, 13, 1, 32)
    assert not [k for k in ours.__dict__ if k.startswith('_nfi')]          # a direct call leaves nothing on the module
    assert a.shape == b.shape == (2, 5 * 13 * 7, 10)
    assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())


@pytest.mark.gpu
def test_refusals(gpu_device):
    from stand_in import StandInGenerator
    model = StandInGenerator(0.55, use_viewdir=True, plane_res=16).to(gpu_device)
    with pytest.raises(TypeError, match='fc1'):
        nfi_gen.attach(model, hip_viewdir_mapper=True)
    with pytest.raises(TypeError, match='use_viewdir'):
        nfi_gen.attach(StandInGenerator(0.55, plane_res=16).to(gpu_device), hip_viewdir_mapper=True)
    nfi_gen.attach(model)          # the default still takes it
    params = [torch.zeros(s) for _, s in ops.VIEWDIR_MAPPER_PARAMS]
    with pytest.raises(RuntimeError, match='GPU'):
        ops.viewdir_mapper_fwd(torch.zeros(4, 3), params)
    with pytest.raises(RuntimeError, match='GPU'):
        ops.viewdir_mapper_bwd(torch.zeros(4, 3), params, torch.zeros(4, 32))
    with pytest.raises(RuntimeError, match='GPU'):
        ops.viewdir_mapper_fwd(torch.zeros(4, 3, device=gpu_device), params)
