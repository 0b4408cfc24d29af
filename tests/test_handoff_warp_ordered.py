"""The ordered backwards of the augmentation warp and of the fused hand-off on the GPU: nfi_affine_warp_bwd_ordered
(ops.affine_warp_bwd(..., ordered=True)) and nfi_torgb_texels_bwd_ordered (ops.torgb_texels_bwd(..., ordered=True)) return
the same bits on every launch - and the right gradients, at the bounds test_neighbours.py and test_handoff.py hold the
atomic entries to against the same float64 references.  Then a whole inversion-style step (producer with the fused
hand-off, render, 15 warped copies) whose every gradient repeats bit for bit."""
import hashlib
import math
import types

import pytest
import torch

from nerf_from_image_amd import _lib, ops
from oracle import nfi_oracle_neighbours as orn
import nerf_from_image_amd.augment as aug
import nerf_from_image_amd.generator as nfi_gen
import nerf_from_image_amd.render as nfi_render

pytestmark = pytest.mark.gpu


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------
# 1. the warp: identity (scale = NULL), zoom-out (many outputs per source pixel), zoom-in, everything outside
# ------------------------------------------------------------------------------------------------
TRANSFORMS = {'identity': (0.0, None, (0.0, 0.0)), 'zoom_out': (math.pi / 4, 0.5, (0.1, -0.05)),
              'zoom_in': (1.0, 2.0, (0.0, 0.0)), 'all_outside': (0.3, 1.0, (5.0, 5.0))}
N, C = 3, 6


def warp_case(name, H, W):
    rot, scale, shift = TRANSFORMS[name]
    g = torch.Generator().manual_seed(H * 1000 + W)
    d = types.SimpleNamespace(rot=torch.full((N,), rot), scale=None if scale is None else torch.full((N,), scale),
                              trans=torch.tensor([shift] * N), x=torch.rand(N, C, H, W, generator=g) * 2 - 1,
                              y=torch.randn(N, C, H, W, generator=g))
    d.y[:, :, H // 4:H // 2 + 1, W // 3:] = 0                  # a block of zeros in the upstream gradient
    return d


def warp_bwd(d, dev, ordered, y=None):
    return ops.affine_warp_bwd((d.y if y is None else y).to(dev), d.rot.to(dev), None if d.scale is None else d.scale.to(dev),
                               d.trans.to(dev), False, ordered=ordered)


@pytest.mark.parametrize('H,W', [(5, 7), (33, 65), (64, 64)])
@pytest.mark.parametrize('name', list(TRANSFORMS))
def test_warp_ordered_backward(gpu_device, name, H, W):
    """Six launches are torch.equal; the result is within test_neighbours.py's bound (1e-4 of the gradient's largest entry)
    of float64 autograd of the oracle's warp_images, and that file's adjoint identity holds with the sums in float64."""
    dev = gpu_device
    d = warp_case(name, H, W)
    first = warp_bwd(d, dev, True)
    for launch in range(1, 6):
        assert torch.equal(warp_bwd(d, dev, True), first), (name, launch)
    x64 = d.x.double().requires_grad_()
    ones = torch.ones(N, dtype=torch.float64)
    ref_out = orn.warp_images(x64, d.rot.double(), ones if d.scale is None else d.scale.double(), d.trans.double(), False)
    ref_g, = torch.autograd.grad((ref_out * d.y.double()).sum(), x64)
    err, scale = (first.cpu().double() - ref_g).abs().max().item(), ref_g.abs().max().item()
    print('%s %dx%d: max err %.3e of %.3e' % (name, H, W, err, scale))
    if name == 'all_outside':
        assert scale == 0 and not first.any()
    else:
        assert scale > 0
    assert err <= 1e-4 * scale
    out = ops.affine_warp(d.x.to(dev), d.rot.to(dev), None if d.scale is None else d.scale.to(dev), d.trans.to(dev), False)
    a, b = (out * d.y.to(dev)).double().sum(), (d.x.to(dev) * first).double().sum()
    assert abs(float(a - b)) <= 1e-6 * abs(float(a)) + 1e-4
    # the white-background flag is accepted and does not enter the adjoint
    assert torch.equal(ops.affine_warp_bwd(d.y.to(dev), d.rot.to(dev), None if d.scale is None else d.scale.to(dev), d.trans.to(dev),
                                           True, ordered=True), first)
    if name == 'zoom_out':
        atomic = {sha(warp_bwd(d, dev, False)) for _ in range(6)}
        print('zoom_out %dx%d: the atomic entry gave %d distinct results in six launches' % (H, W, len(atomic)))


def test_warp_ordered_through_augment(gpu_device):
    """augment.configure(..., deterministic_backward=True) reaches the warp's backward; the forward is the same launch."""
    dev = gpu_device
    d = warp_case('zoom_out', 33, 65)
    tform = (d.rot.to(dev), d.scale.to(dev), d.trans.to(dev))
    cfg = types.SimpleNamespace(supervise_alpha=False), {'white_background': True}
    try:
        got = {}
        for flag in (False, True):
            aug.configure(*cfg, deterministic_backward=flag)
            x = d.x.to(dev).requires_grad_()
            out, _, _ = aug.augment(x, None, None, 1.0, cached_tform=tform)
            got[flag] = out.detach(), torch.autograd.grad((out * d.y.to(dev)).sum(), x)[0]
        assert torch.equal(got[True][0], got[False][0])
        assert torch.equal(got[True][1], warp_bwd(d, dev, True))
    finally:
        aug.configure(*cfg)


# ------------------------------------------------------------------------------------------------
# 2. the hand-off backward
# ------------------------------------------------------------------------------------------------
# (1, 16, 8): one wave tile, one block; (2, 144, 40): the second tk0 pass with ntk = 1, a last channel group of one tile, two
# ragged blocks; (2, 32, 96): more than 256 wanted blocks, so the weight kernel's grid-stride loop runs
SHAPES = [(1, 16, 8), (2, 144, 40), (2, 32, 96)]
_handoff_cache = {}


def handoff_case(B, Cin, R):
    """Inputs and the float64 gradients of test_handoff.test_torgb_texels_backward_against_float64_autograd's restatement,
    with and without a previous image; computed once per shape."""
    if (B, Cin, R) not in _handoff_cache:
        g = torch.Generator().manual_seed(B * 1000 + Cin + R)
        t = dict(x=torch.randn(B, Cin, R, R, generator=g), s=torch.randn(B, Cin, generator=g) / Cin ** 0.5,
                 w=torch.randn(96, Cin, generator=g), bias=torch.randn(96, generator=g),
                 prev=torch.randn(B, 96, R // 2, R // 2, generator=g), up=torch.randn(B, 96, R, R, generator=g))
        ref = {}
        for has_prev in (False, True):
            leaves = [t[k].double().requires_grad_() for k in ('x', 's', 'w', 'bias')] + ([t['prev'].double().requires_grad_()] if has_prev else [])
            out = orn.torgb_upsample_add(leaves[0], leaves[1], leaves[2].view(96, Cin, 1, 1), leaves[3], leaves[4] if has_prev else None)
            gr = torch.autograd.grad((out * t['up'].double()).sum(), leaves)
            ref[has_prev] = dict(zip(('g_x', 'g_styles', 'g_weight', 'g_bias', 'g_previous_image'), gr))
        _handoff_cache[B, Cin, R] = t, ref
    return _handoff_cache[B, Cin, R]


def handoff_bwd(t, dev, has_prev, want_weight, ordered):
    return ops.torgb_texels_bwd(t['up'].to(dev), t['x'].to(dev), t['s'].to(dev), t['w'].to(dev), t['prev'].to(dev) if has_prev else None,
                                want_weight=want_weight, ordered=ordered)


@pytest.mark.parametrize('want_weight', [True, False], ids=['weight', 'no_weight'])
@pytest.mark.parametrize('has_prev', [True, False], ids=['prev', 'no_prev'])
@pytest.mark.parametrize('B,Cin,R', SHAPES)
def test_handoff_ordered_backward(gpu_device, B, Cin, R, has_prev, want_weight):
    """Six launches are torch.equal on every output; g_x and g_previous_image are the atomic entry's bits; every output is
    within test_handoff.py's bound (2e-5 of the gradient's largest entry) of the float64 restatement."""
    dev = gpu_device
    t, ref = handoff_case(B, Cin, R)
    first = handoff_bwd(t, dev, has_prev, want_weight, True)
    keys = ['g_x', 'g_styles'] + (['g_weight', 'g_bias'] if want_weight else []) + (['g_previous_image'] if has_prev else [])
    assert sorted(first) == sorted(keys)
    for launch in range(1, 6):
        again = handoff_bwd(t, dev, has_prev, want_weight, True)
        for k in keys:
            assert torch.equal(again[k], first[k]), (k, launch)
    atomic = handoff_bwd(t, dev, has_prev, want_weight, False)
    for k in ('g_x', 'g_previous_image'):
        if k in first:
            assert torch.equal(first[k], atomic[k]), k
    for k in keys:
        b = ref[has_prev][k]
        assert first[k].shape == b.shape, k
        err = (first[k].cpu().double() - b).abs().max().item()
        print('%s %s: max err %.3e of %.3e' % ((B, Cin, R), k, err, b.abs().max().item()))
        assert err <= 2e-5 * b.abs().max().item(), (k, err, b.abs().max().item())


@pytest.mark.parametrize('B,Cin,R', SHAPES)
def test_handoff_workspace_needs_no_zeroing(gpu_device, B, Cin, R):
    """Through the raw entry: a workspace full of NaN before each of two calls, and the results are those of ops'."""
    dev = gpu_device
    t, _ = handoff_case(B, Cin, R)
    want = handoff_bwd(t, dev, True, True, True)
    d = {k: v.to(dev) for k, v in t.items()}
    g = d['up'].contiguous(memory_format=torch.channels_last)
    for call in range(2):
        out = {'g_x': torch.empty_like(d['x']), 'g_styles': torch.empty_like(d['s']), 'g_weight': torch.empty_like(d['w']),
               'g_bias': torch.empty_like(d['bias']), 'g_previous_image': torch.empty_like(d['prev'])}
        args = dict(n_scenes=B, in_channels=Cin, resolution=R, x=d['x'], styles=d['s'], weight=d['w'], previous_image=d['prev'],
                    g_texels=g, **out)
        n_ws = _lib.struct_query('nfi_torgb_texels_bwd_ordered_workspace_bytes', 'nfi_torgb_args', **args)
        ws = torch.full((n_ws // 4,), float('nan'), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.call_struct('nfi_torgb_texels_bwd_ordered', 'nfi_torgb_args', torch.cuda.current_stream(dev).cuda_stream, ws, n_ws, **args)
        for k in out:
            assert torch.equal(out[k], want[k]), (k, call)


# ------------------------------------------------------------------------------------------------
# 3. a whole step: producer (fused hand-off) -> render -> 15 warped copies of cat(rgb, target) -> a fixed-weight loss
# ------------------------------------------------------------------------------------------------
STEP_NAMES = ['z', 'cam2world', 'focal', 'torgb.weight', 'torgb.bias', 'torgb.affine.weight', 'torgb.affine.bias', 'w1', 'b1', 'w2', 'b2']


def step(dev, ordered):
    from stand_in import StandInGenerator, StyleLikeSynthesis, look_at_cameras
    torch.manual_seed(4)
    model = StandInGenerator(0.55, attention_values=10, use_sdf=True, plane_res=32)
    model.synthesis_network = StyleLikeSynthesis(32, channels=32)
    model = model.to(dev).train()
    nfi_gen.attach(model, fused_handoff=True, deterministic_backward=ordered)
    cfg = types.SimpleNamespace(use_viewdir=False, use_sdf=True, attention_values=10, fine_sampling=True, supervise_alpha=False)
    dcfg = {'scene_range': 0.55, 'white_background': True}
    render = nfi_render.make_render(cfg, dcfg, deterministic_backward=ordered)
    aug.configure(cfg, dcfg, deterministic_backward=ordered)
    g = torch.Generator().manual_seed(2)
    B, H, W, S, copies = 2, 16, 16, 16, 15
    cam = look_at_cameras(B, 1.6, g).to(dev).requires_grad_()
    focal = torch.full((B,), 1.0254, device=dev).requires_grad_()
    z = torch.randn(B, 512, generator=g).to(dev).requires_grad_()
    target = torch.rand(B, 3, H, W, generator=g).to(dev)
    weights = torch.randn(copies * B, 6, H, W, generator=g).to(dev)
    torch.manual_seed(33)                                     # the render's noise and the augmentation's draws
    rgb = render(model, H, W, cam, focal, None, None, z, S)[0]
    both = torch.cat([rgb.permute(0, 3, 1, 2), target], dim=1).repeat(copies, 1, 1, 1)
    warped, _, _ = aug.augment(both, None, None, 0.8)
    loss = (warped * weights).sum()
    last, dec = model.synthesis_network.b32, model.decoder.net
    leaves = [z, cam, focal, last.torgb.weight, last.torgb.bias, last.torgb.affine.lin.weight, last.torgb.affine.lin.bias,
              dec[0].weight, dec[0].bias, dec[2].weight, dec[2].bias]
    return (rgb.detach(), warped.detach()), torch.autograd.grad(loss, leaves)


def test_whole_step_repeats_bit_for_bit(gpu_device):
    """Four runs with the same seeds and every switch on (the producer on MIOpen's deterministic solvers): the gradients of
    the latents, camera, focal, the last block's torgb weight / bias / affine and the decoder are torch.equal.  With the
    switches off the forward outputs are the same bits: the option belongs to the backward alone."""
    dev = gpu_device
    before = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        fwd, first = step(dev, True)
        assert all(float(t.abs().max()) > 0 for t in first)
        for run in range(1, 4):
            fwd_again, again = step(dev, True)
            assert all(torch.equal(a, b) for a, b in zip(fwd_again, fwd)), run
            for n, a, b in zip(STEP_NAMES, again, first):
                assert torch.equal(a, b), (n, run)
        fwd_default, default = step(dev, False)
        assert all(torch.equal(a, b) for a, b in zip(fwd_default, fwd))
        for n, a, b in zip(STEP_NAMES, first, default):
            print('grad %-20s ordered vs default rel %.3e' % (n, float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))))
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = before
        aug.configure(types.SimpleNamespace(supervise_alpha=False), {'white_background': True})
