"""The regulariser branch's distance-plus-gradient operator, nfi_sdf_gradient_fwd / nfi_sdf_gradient_bwd
(csrc/nfi_regulariser.inc), element by element against float64.

The reference is oracle.nfi_oracle.sdf_and_gradient on the CPU, differentiated by autograd in float64:
    loss = sum(sdf * u_d) + sum(gradient * u_g),   random upstream u_d [B,P], u_g [B,P,3]
and its gradients with respect to planes, w1, b1, w2, b2 - the backward kernel is the reference's DOUBLE backward.
Every scene is built from a seed (band-limited planes + 0.1 noise, as test_kernel_matrix.field_scene).  Points are placed
by TEXEL coordinate: an integer cell in [0, res-2] and a fraction in [margin, 1-margin] per axis, p = ((cell + frac) /
(res-1) * 2 - 1) * r in float64 with r the fp32 value of scene_range, rounded to fp32.  That keeps every point strictly
inside the cube (the kernel's documented precondition; outside it and on the upper face the kernel and
lib/ops.grid_sample2d differ by design) and off the texel nodes, where d sdf / dx jumps and an fp32 kernel and a float64
oracle may legitimately pick different cells.  The one exception is the `nodes` case, whose coordinates are exact in fp32.

Bounds (none invented here):
    sdf                   1e-5 x max(1, max |ref|)                                           test_field_row's, same output
    gradient              max(3e-5, 4 x the float32 oracle's own distance) x max |ref|       test_render_row's normal map /
                                                                                             test_render_backward_end_to_end's 4 x rule
    each backward output  max(5e-4, 4 x the float32 oracle's own distance) x its max |ref|   test_field_bwd_row's, same decoder
    same sum, other order 2e-5 x max |ref|                                                    test_field_bwd_row's
test_inputs_are_well_conditioned_for_the_reference (CPU) holds the float32 oracle within 1e-5 of the float64 oracle for
every case, so a figure over its bound on the GPU is the kernel's doing.

What the cases reach that the scalar-loss tests (test_host_api_gpu.test_regulariser_outputs*, test_reference_gpu) do not:
more than one 64-point chunk per wave in the backward (dW1 / db1 / dw2 carried over, sticky_scale rescaling dW1, LDS tiles
reused), upstream gradients at 1e-7 and 3e4 and changing by many decades from chunk to chunk and from point to point,
ragged tails (P = 1, 15, 17, 63, 65, 5003), NULL g_sdf / g_gradient, the accumulate-into contract, plane sizes 2, 3, 9, 17,
24, 257, 385 and 769, scene_range 0.5 and 2.0, a saturated decoder, the interleaved texel layout, and points on the nodes.

Every test prints each figure with its bound and the float32 oracle's own distance beside it; DESIGN.md section 2,
"Regulariser operator", keeps the largest per quantity.  Conditioning of the inputs (float32 against float64 oracle,
largest over the cases): sdf 8.5e-7, gradient 8.5e-6, planes 7.7e-6, w1 6.3e-6, b1 3.4e-6, w2 7.0e-6, b2 8.6e-7, all at
res = 257; every other case stays below 1.9e-6.
"""
import collections
import functools

import pytest
import torch
import torch.nn.functional as F

from parity_util import grad_close
from nerf_from_image_amd import _lib, ops
from oracle import nfi_oracle as orc

Case = collections.namedtuple('Case', 'name B P res scene_range n_out w1_gain upstream margin placement lattice backward')


def case(name, B, P, res, scene_range, n_out, w1_gain=1.0, upstream=1.0, margin=0.02, placement='uniform', lattice=False, backward=True):
    return Case(name, B, P, res, scene_range, n_out, w1_gain, upstream, margin, placement, lattice, backward)


CASES = [
    case('base', 2, 200, 24, 0.55, 11),
    case('one_point_res2', 1, 1, 2, 0.55, 4),
] + [
    # tile (16) and chunk (64) boundaries; n_out = 33 is the view-direction decoder's second layer
    case('tail_P%d' % P, 2, P, 3, 2.0, 33) for P in (15, 16, 17, 63, 64, 65)
] + [
    # backward: 256 / 16 = 16 blocks = 64 waves for 79 chunks, so 15 waves do two; the last tile has 11 live points
    case('two_chunks_per_wave', 16, 5003, 9, 0.55, 11),
    # forward: max(16, 1024 / 16) = 64 blocks = 256 waves for 266 chunks
    case('fwd_more_chunks_than_waves', 16, 17000, 9, 0.55, 4, backward=False),
    # res = 257: cells up to 255 and texel nodes up to 256 on every axis, a quarter of the points in cells >= 250
    case('res257', 1, 777, 257, 2.0, 11, margin=0.05, placement='high_quarter'),
    # cells ABOVE 255 (bit 8, and with res = 769 bit 9, of the 10-bit packed index).  From res = 258 on the fp32 rounding of the
    # texel coordinate alone moves the float32 oracle 1.3e-5 ... 2.9e-5 from the float64 one (6e-5 at res = 1024, where
    # scene_range = 0.55 leaves no way round it: that case of the issue is left out), so these two put the points on a
    # lattice whose texel coordinate u = 3 n / 64 is EXACT in fp32 (res - 1 = 3 * 2^k, scene_range a power of two)
    case('lattice_res385', 1, 777, 385, 2.0, 11, margin=0.05, placement='high_quarter', lattice=True),
    case('lattice_res769', 1, 1025, 769, 2.0, 4, margin=0.05, placement='ends', lattice=True, backward=False),
    # the issue's w1 x 8: pre-activations reach +-13.4 only (their spread is 3.3, so 20 is six sigma: no seed gets there) ...
    case('w1_x8', 2, 200, 24, 0.55, 11, w1_gain=8.0),
    # ... so the saturated case takes w1 x 16: some above 20 (the soft-plus's linear branch), over a thousand below -10
    case('saturated_decoder', 2, 200, 24, 0.55, 11, w1_gain=16.0),
    case('upstream_1e-7', 2, 200, 24, 0.55, 11, upstream=1e-7),
    case('upstream_3e4', 2, 200, 24, 0.55, 11, upstream=3e4),
    case('upstream_per_chunk', 16, 5003, 9, 0.55, 11, upstream='chunk'),
    case('upstream_per_point', 16, 5003, 9, 0.55, 11, upstream='point'),
    # p = (k - 8) / 16 with res = 17 and scene_range = 0.5: exact in fp32, u = k exactly, k in [0, 15]
    case('nodes', 2, 40, 17, 0.5, 11, placement='nodes'),
]
CASE = {c.name: c for c in CASES}
# seed = 9000 + index of the case, unless listed here (chosen so that the float32 oracle stays well inside 1e-5)
RESEED = {'res257': 9200}
PARAMS = ('planes', 'w1', 'b1', 'w2', 'b2')


def seed_of(c):
    return RESEED[c.name] if c.name in RESEED else 9000 + CASES.index(c)


def range_of(c):
    return float(torch.tensor(c.scene_range, dtype=torch.float32))


def big(c):
    """Planes that stay float32 on the CPU (float64 planes of res = 769 would take 0.45 GB; the oracle's gather promotes)."""
    return c.res >= 512


def scene(c):
    """dict(planes, w1, b1, w2, b2, x, u_d, u_g), float32 on the CPU, from the case's seed alone."""
    g = torch.Generator().manual_seed(seed_of(c))
    B, P, res, r = c.B, c.P, c.res, range_of(c)
    k = min(res, 8)
    low = torch.randn(B * 3, 32, k, k, generator=g)
    planes = F.interpolate(low, size=(res, res), mode='bilinear', align_corners=True)
    planes.add_(torch.randn(B * 3, 32, res, res, generator=g), alpha=0.1)
    t = dict(planes=planes.view(B, 3, 32, res, res), w1=torch.randn(64, 32, generator=g) * c.w1_gain,
             b1=0.3 * torch.randn(64, generator=g), w2=torch.randn(c.n_out, 64, generator=g), b2=0.3 * torch.randn(c.n_out, generator=g))
    if c.placement == 'nodes':
        node = torch.randint(0, res - 1, (B, P, 3), generator=g)
        node[0, :3] = torch.tensor([[0, 0, 0], [15, 15, 15], [0, 15, 7]])          # the lower face and the last cell
        node[1, :2] = torch.tensor([[3, 0, 15], [15, 8, 0]])
        t['x'] = ((node.double() - 8) / 16).float()
    else:
        cell = torch.randint(0, res - 1, (B, P, 3), generator=g)
        if c.placement == 'ends':               # half the points in the first two and last two cells of each axis
            cell[:, :P // 2] = torch.tensor([0, 1, res - 3, res - 2])[torch.randint(0, 4, (B, P // 2, 3), generator=g)]
        elif c.placement == 'high_quarter':
            cell[:, :P // 4 + 1] = torch.randint(250, res - 1, (B, P // 4 + 1, 3), generator=g)
        frac = c.margin + (1 - 2 * c.margin) * torch.rand(B, P, 3, generator=g, dtype=torch.float64)
        if c.lattice:
            n = torch.round((cell.double() + frac) * 64 / 3)               # u = 3 n / 64, within 1 / 43 of the drawn one
            t['x'] = ((n * 2 / (64 * (res - 1) // 3) - 1) * r).float()
        else:
            t['x'] = (((cell.double() + frac) / (res - 1) * 2 - 1) * r).float()
    u_d, u_g = torch.randn(B, P, generator=g), torch.randn(B, P, 3, generator=g)
    if c.upstream == 'chunk':
        s = (10.0 ** (torch.rand(B, (P + 63) // 64, generator=g) * 13 - 9)).repeat_interleave(64, 1)[:, :P]
    elif c.upstream == 'point':
        s = 10.0 ** (torch.rand(B, P, generator=g) * 13 - 9)
    else:
        s = torch.full((B, P), float(c.upstream))
    t['u_d'], t['u_g'] = u_d * s, u_g * s[..., None]
    return t


def oracle(c, t, dtype, use_d=True, use_g=True):
    """sdf, gradient and (c.backward) the gradients of the loss w.r.t. planes, w1, b1, w2, b2, all in `dtype`."""
    L = {k: (t[k] if k == 'planes' and big(c) else t[k].to(dtype)).detach().requires_grad_(c.backward) for k in PARAMS}
    d, g = orc.sdf_and_gradient(L['planes'], L['w1'], L['b1'], L['w2'], L['b2'], t['x'].to(dtype), range_of(c), create_graph=c.backward)
    out = dict(sdf=d.detach(), gradient=g.detach())
    if c.backward:
        loss = (d * t['u_d'].to(dtype)).sum() * float(use_d) + (g * t['u_g'].to(dtype)).sum() * float(use_g)
        out.update(zip(PARAMS, torch.autograd.grad(loss, [L[k] for k in PARAMS])))
    return out


@functools.lru_cache(maxsize=None)
def reference(name, use_d=True, use_g=True):
    """(inputs, float64 oracle, float32 oracle) of a case, computed once and shared (read-only) by the tests."""
    c = CASE[name]
    t = scene(c)
    r64, r32 = oracle(c, t, torch.float64, use_d, use_g), oracle(c, t, torch.float32, use_d, use_g)
    if big(c):
        del t['planes']                        # 0.4 GB; the GPU test builds them again
    return t, r64, r32


def rel(a, ref):
    return float((a.double() - ref.double()).abs().max()) / float(ref.double().abs().max().clamp_min(1e-300))


def preactivations(c, t):
    """h = W1' f + b1 of every point, float64."""
    x = t['x'].double() / range_of(c)
    p = t['planes'].double()
    feats = (orc._bilinear_double_differentiable(p[:, 0], x[..., 0], x[..., 1]) + orc._bilinear_double_differentiable(p[:, 1], x[..., 0], x[..., 2]) +
             orc._bilinear_double_differentiable(p[:, 2], x[..., 1], x[..., 2])) / 3
    gw1, gb1, _, _ = orc.decoder_params(t['w1'].double(), t['b1'].double(), t['w2'].double(), t['b2'].double())
    return F.linear(feats.transpose(-2, -1), gw1, gb1)


def saturation_of(c, t):
    h = preactivations(c, t)
    return float(h.max()), float(h.min())


def test_inputs_are_well_conditioned_for_the_reference():
    """A condition on the INPUTS, so that a figure over its bound on the GPU is the kernel's doing: for every case the
    float32 oracle is within 1e-5 of the float64 oracle - sdf and gradient of every point (none is left out) and all five
    parameter / plane gradients, each relative to its own largest entry.  Every point lies strictly inside the cube and,
    the `nodes` case apart, at least half its margin away from every texel node after rounding to fp32; the saturated case
    really has pre-activations above 20 (the soft-plus's linear branch) and below -10."""
    bad = []
    worst = collections.defaultdict(float)
    for c in CASES:
        t, r64, r32 = reference(c.name)
        figs = {k: rel(r32[k], r64[k]) for k in r64}
        print('%-28s seed %d  %s' % (c.name, seed_of(c), '  '.join('%s %.1e' % kv for kv in figs.items())))
        for k, e in figs.items():
            worst[k] = max(worst[k], e)
            if not e <= 1e-5:
                bad.append((c.name, k, e))
        r = range_of(c)
        # (the lower face, x = -r, is reached by the `nodes` case alone)
        assert tuple(t['x'].shape) == (c.B, c.P, 3) and float(t['x'].max()) < r and float(t['x'].min()) >= -r, c.name
        u = (t['x'].double() / r + 1) / 2 * (c.res - 1)
        fr = u - torch.floor(u)
        if c.placement == 'nodes':
            assert float(fr.abs().max()) == 0.0 and float(u.max()) <= c.res - 2 and float(u.min()) == 0.0, c.name
        else:
            assert c.margin / 2 < float(fr.min()) and float(fr.max()) < 1 - c.margin / 2, (c.name, float(fr.min()), float(fr.max()))
        if c.lattice:
            u32 = (t['x'] / torch.tensor(r) + 1) / 2 * (c.res - 1)            # as the kernel and the float32 oracle compute it
            assert torch.equal(u32.double(), u) and torch.equal(u * 64 / 3, torch.round(u * 64 / 3)), c.name
        if c.placement in ('high_quarter', 'ends'):
            cells = torch.floor(u)
            assert float(cells.max()) == c.res - 2 and float(cells.min()) == 0, c.name
            assert float((cells >= 250).all(dim=-1).float().mean()) >= (0.25 if c.placement == 'high_quarter' else 0.1), c.name
    hi, lo = saturation_of(CASE['saturated_decoder'], reference('saturated_decoder')[0])
    print('saturated_decoder: pre-activations in [%.1f, %.1f]' % (lo, hi))
    assert hi > 20 and lo < -10, (hi, lo)
    print('largest float32 - float64 difference: ' + '  '.join('%s %.1e' % kv for kv in worst.items()))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------
# on the GPU
# ------------------------------------------------------------------------------------------------
def texels_of(t, dev, interleaved=False):
    texels = ops.planes_to_texels(t['planes'].to(dev))
    return texels.permute(0, 2, 3, 1, 4).contiguous() if interleaved else texels


def hip_fwd(c, t, texels):
    dev = texels.device
    return ops.sdf_gradient_fwd(t['x'].to(dev), texels, t['w1'].to(dev), t['b1'].to(dev), t['w2'].to(dev), t['b2'].to(dev), range_of(c))


def hip_bwd(c, t, texels, g_sdf='u_d', g_gradient='u_g'):
    """g_sdf / g_gradient: a key of t, a tensor, or None (a NULL pointer)."""
    dev = texels.device
    up = lambda v: None if v is None else (t[v] if isinstance(v, str) else v).to(dev)
    out = ops.sdf_gradient_bwd(t['x'].to(dev), texels, t['w1'].to(dev), t['b1'].to(dev), t['w2'].to(dev), t['b2'].to(dev), range_of(c),
                               up(g_sdf), up(g_gradient))
    return {'planes': ops.texel_grad_to_planes(out['g_texels']), 'w1': out['g_w1'], 'b1': out['g_b1'], 'w2': out['g_w2'], 'b2': out['g_b2']}


def check_forward(what, sdf, gradient, r64, r32):
    ref = r64['sdf']
    tol = 1e-5 * max(1.0, float(ref.abs().max()))
    e = float((sdf.detach().double().cpu() - ref).abs().max())
    print('%-60s max %.3e (bound %.1e, float32 oracle %.3e)' % (what + ': sdf', e, tol, float((r32['sdf'].double() - ref).abs().max())))
    assert sdf.shape == ref.shape and torch.isfinite(sdf).all() and e <= tol, (what, e, tol)
    grad_close(gradient, r64['gradient'], max(3e-5, 4 * rel(r32['gradient'], r64['gradient'])), what + ': gradient', r32['gradient'])


def check_backward(what, got, r64, r32):
    assert float(r64['planes'].abs().max()) > 0
    for k in PARAMS:
        grad_close(got[k], r64[k], max(5e-4, 4 * rel(r32[k], r64[k])), '%s: grad %s' % (what, k), r32[k])


@pytest.mark.gpu
@pytest.mark.parametrize('name', [c.name for c in CASES])
def test_operator_case(gpu_device, name):
    """Forward and (unless the case is forward-only) all five gradients of one case against the float64 oracle.

    `base` runs in both texel layouts.  The `tail_P*` cases have the view-direction decoder's 33-row second layer: rows
    1.. of g_w2 and g_b2 stay exactly zero.  `upstream_per_chunk` / `upstream_per_point` draw the upstream scale as
    10^U(-9, 4) per 64-point chunk / per point, so consecutive chunks of one wave differ by many decades in both directions.
    Every gradient is compared relative to its own largest entry, so these two cannot see a corrupted contribution from a
    chunk whose scale lies decades below the largest; what they test is that a rescale of the sticky dW1 scale does not
    damage what is already accumulated (and that small contributions after a large one do not disturb it)."""
    c = CASE[name]
    t, r64, r32 = reference(name)
    if big(c):
        t = dict(t, planes=scene(c)['planes'])
    if name == 'saturated_decoder':
        hi, lo = saturation_of(c, t)
        assert hi > 20 and lo < -10, (hi, lo)                  # else the case proves nothing
    for interleaved in ((False, True) if name == 'base' else (False,)):
        what = name + (' (interleaved)' if interleaved else '')
        texels = texels_of(t, gpu_device, interleaved)
        sdf, gradient = hip_fwd(c, t, texels)
        check_forward(what, sdf, gradient, r64, r32)
        if not c.backward:
            continue
        got = hip_bwd(c, t, texels)
        check_backward(what, got, r64, r32)
        if c.n_out == 33:
            assert not got['w2'][1:].any() and not got['b2'][1:].any(), what


@pytest.mark.gpu
def test_null_upstream_gradients(gpu_device):
    """g_gradient == NULL equals the launch with an all-zero g_gradient (2e-5: same sum, other atomic order) and matches
    the oracle with that term left out of the loss; likewise g_sdf == NULL; both NULL is refused with a message."""
    c = CASE['base']
    t = reference('base')[0]
    texels = texels_of(t, gpu_device)
    for null, kw_null, kw_zero, ref_kw in (
            ('g_gradient', dict(g_gradient=None), dict(g_gradient=torch.zeros_like(t['u_g'])), dict(use_g=False)),
            ('g_sdf', dict(g_sdf=None), dict(g_sdf=torch.zeros_like(t['u_d'])), dict(use_d=False))):
        got, zero = hip_bwd(c, t, texels, **kw_null), hip_bwd(c, t, texels, **kw_zero)
        _, r64, r32 = reference('base', **ref_kw)
        for k in PARAMS:
            grad_close(got[k], zero[k], 2e-5, '%s = NULL vs zeros: grad %s' % (null, k))
        check_backward('%s = NULL' % null, got, r64, r32)
    with pytest.raises(RuntimeError, match='no upstream gradient'):
        hip_bwd(c, t, texels, g_sdf=None, g_gradient=None)


@pytest.mark.gpu
def test_backward_accumulates_into_its_outputs(gpu_device):
    """The ABI's contract for g_texels, g_w1, g_b1, g_w2, g_b2: after one launch each holds its O(1) random pre-fill plus
    the gradient that a launch into zeros gives, to 2e-5 of that gradient's largest entry."""
    dev = gpu_device
    c = CASE['base']
    t = reference('base')[0]
    texels = texels_of(t, dev)
    d = {k: t[k].to(dev) for k in ('x', 'w1', 'b1', 'w2', 'b2', 'u_d', 'u_g')}
    zero = ops.sdf_gradient_bwd(d['x'], texels, d['w1'], d['b1'], d['w2'], d['b2'], range_of(c), d['u_d'], d['u_g'])
    g = torch.Generator().manual_seed(77)
    shapes = {'g_texels': texels.shape, 'g_w1': (64, 32), 'g_b1': (64,), 'g_w2': (c.n_out, 64), 'g_b2': (c.n_out,)}
    pre = {k: torch.randn(*s, generator=g) for k, s in shapes.items()}
    out = {k: v.to(dev) for k, v in pre.items()}
    with torch.cuda.device(dev):
        _lib.call_struct('nfi_sdf_gradient_bwd', 'nfi_sdf_gradient_args', torch.cuda.current_stream(dev).cuda_stream,
                         n_scenes=c.B, points_per_scene=c.P, points=d['x'], texels=texels, plane_res=c.res,
                         texel_layout=ops.texel_layout_of(texels), scene_range=range_of(c), w1=d['w1'], b1=d['b1'], w2=d['w2'],
                         b2=d['b2'], g_sdf=d['u_d'], g_gradient=d['u_g'], **out)
    for k in shapes:
        assert float(zero[k].abs().max()) > 0.01, k          # so that the pre-fill's fp32 rounding stays far below the bound
        grad_close(out[k].double().cpu() - pre[k].double(), zero[k], 2e-5, 'accumulated %s - pre-fill vs launch into zeros' % k)
    assert torch.equal(out['g_w2'][1:].cpu(), pre['g_w2'][1:]) and torch.equal(out['g_b2'][1:].cpu(), pre['g_b2'][1:])
