"""The ordered backward on the GPU: nfi_field_bwd_args.scatter_mode 2, nfi_raygen_bwd_ordered and the render option
deterministic_backward return the same bits on every launch - and the right gradients: against float64 autograd of the
oracle at the suite's bounds, and against the atomic scatter (mode 0) at the bound the binned scatter is held to."""
import copy
import hashlib
import types

import pytest
import torch

from conftest import load_golden
from nerf_from_image_amd import _lib, field_backward as fb, ops
from oracle import nfi_oracle as orc
from stand_in import StandInGenerator, look_at_cameras, _Decoder
import nerf_from_image_amd.generator as nfi_gen
import nerf_from_image_amd.render as nfi_render
import test_hip_backward as thb
from test_hip_backward import rel_close

pytestmark = pytest.mark.gpu

R_SCENE = 0.55


def scatter_case(dev, P, res, B=2, A=10, use_sdf=True, tex=ops.TEXEL_F32, interleaved=False):
    """The inputs of test_binned_scatter_matches_atomic_scatter: points beyond the cube, a crowd of a quarter of scene 0's
    points in a few cells, no upstream gradient for the second half of the last scene's points."""
    g = torch.Generator().manual_seed(500 + P)
    planes = torch.randn(B, 3, 32, res, res, generator=g).to(dev)
    dec = _Decoder(1 + A if A > 0 else 4, g).to(dev)
    w1, b1, w2, b2 = (t.detach() for t in (dec.net[0].weight, dec.net[0].bias, dec.net[2].weight, dec.net[2].bias))
    x = ((torch.rand(B, P, 3, generator=g) * 2 - 1) * R_SCENE * 1.15).to(dev)
    x[0, : P // 4] *= 0.05
    att = (torch.rand(B, A, 3, generator=g) * 2 - 1).to(dev) if A > 0 else None
    beta, alpha = torch.tensor([0.12], device=dev), torch.tensor([0.3], device=dev)
    g_sig, g_rgb = torch.randn(B, P, generator=g).to(dev), torch.randn(B, P, 3, generator=g).to(dev)
    g_sig[B - 1, P // 2:] = 0
    g_rgb[B - 1, P // 2:] = 0
    texels = ops.planes_to_texels(planes, tex)
    if interleaved:
        texels = texels.permute(0, 2, 3, 1, 4).contiguous()
    image = ops.decoder_pack(w1, b1, w2, b2, A, tex)
    args = (x, texels, image, w1, w2, R_SCENE, A, att, use_sdf, beta if use_sdf else None, alpha if use_sdf else None, g_sig, g_rgb)
    return args


def sha(t):
    return hashlib.sha1(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------
# 1. repeats bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,P,kw,ray_order', [
    (2, 8229, {}, None),                              # 129 chunks: several waves and blocks add to every parameter gradient
    (1, 64, {}, None),                                # the recorded case: 8 plane-gradient hashes in 8 launches of mode 1
    (2, 8229, dict(interleaved=True), None),
    (2, 8229, dict(tex=ops.TEXEL_F16), None),
    (2, 8229, dict(A=0, use_sdf=False), None),
    (2, 16 * 8 * 64, {}, (64, 8)),                    # the ray-order hint: 16 x 8 rays of 64 samples, 8-pixel tiles
])
def test_ordered_mode_repeats_bit_for_bit(gpu_device, B, P, kw, ray_order):
    args = scatter_case(gpu_device, P, 24, B=B, **kw)
    run = lambda mode: fb.field_query_bwd(*args, want_points=True, scatter_mode=mode, ray_order=ray_order)
    first = {k: v.clone() for k, v in run(2).items()}
    want = {'g_texels', 'g_w1', 'g_b1', 'g_w2', 'g_b2', 'g_points'} | ({'g_attention_values'} if args[6] > 0 else set()) | \
           ({'g_beta', 'g_alpha'} if args[8] else set())
    assert set(first) == want
    assert float(first['g_texels'].abs().max()) > 0 and float(first['g_w1'].abs().max()) > 0
    for _ in range(5):
        again = run(2)
        for k in first:
            assert torch.equal(again[k], first[k]), k
    # (for the record only: how many different plane gradients the binned mode gives for these inputs)
    print('mode 1: %d distinct g_texels in 6 launches' % len({sha(run(1)['g_texels']) for _ in range(6)}))


# ------------------------------------------------------------------------------------------------
# 2. the right answer
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def ordered_sampler(monkeypatch):
    """test_hip_backward's float64 comparison, with the sampler closure's backward in the ordered mode."""
    real = nfi_gen.make_sampler
    seen = []

    def make(*a, **k):
        seen.append(1)
        return real(*a, deterministic_backward=True, **k)
    monkeypatch.setattr(thb.nfi_gen, 'make_sampler', make)
    modes = []
    real_bwd = fb.field_query_bwd

    def spy(*a, **k):
        modes.append(k.get('scatter_mode'))
        return real_bwd(*a, **k)
    monkeypatch.setattr(fb, 'field_query_bwd', spy)
    yield modes
    assert seen and modes and all(m == 2 for m in modes), (seen, modes)


@pytest.mark.parametrize('A,use_sdf,P,scale', [(10, True, 200, None), (0, False, 70, None), (10, True, 64, None),
                                               (10, True, 200, 'mixed')])
def test_ordered_mode_against_the_float64_oracle(gpu_device, ordered_sampler, A, use_sdf, P, scale):
    """Every gradient of the sampler closure within 5e-4 of the gradient's maximum (rel_close), the cases of
    test_field_query_backward and the 'mixed' case of test_field_query_backward_at_any_gradient_scale."""
    thb._field_query_backward_case(gpu_device, A, use_sdf, P, scale)


_mode0 = {}


@pytest.mark.parametrize('P,res', [(5000, 24), (333, 9), (3, 2), (20000, 17), (9000, 600), (70000, 64)])
def test_ordered_mode_matches_atomic_scatter(gpu_device, P, res):
    """Every key within 2e-5 of its maximum of mode 0: the bound test_binned_scatter_matches_atomic_scatter holds mode 1 to on
    these inputs (the smallest plane, plane sides off the tile size, empty cells, points outside the cube and on its faces,
    runs of thousands of points in one cell)."""
    args = scatter_case(gpu_device, P, res)
    a = fb.field_query_bwd(*args, want_points=True, scatter_mode=0)
    b = fb.field_query_bwd(*args, want_points=True, scatter_mode=2)
    assert a['g_texels'].abs().max() > 0 and set(a) == set(b)
    for k in a:
        scale = float(a[k].abs().max().clamp_min(1e-12))
        print('P %d res %d: %-20s rel %.3e' % (P, res, k, float((b[k] - a[k]).abs().max()) / scale))
    for k in a:
        rel_close(b[k], a[k], 'ordered vs atomic ' + k, 2e-5)


# ------------------------------------------------------------------------------------------------
# 3. accumulate contract, through the raw ABI
# ------------------------------------------------------------------------------------------------
def test_ordered_mode_adds_into_the_callers_buffers(gpu_device):
    dev = gpu_device
    B, P, res, A = 2, 8229, 24, 10
    x, texels, image, w1, w2, r, _, att, _, beta, alpha, g_sig, g_rgb = scatter_case(dev, P, res)
    shapes = dict(g_texels=tuple(texels.shape), g_w1=(64, 32), g_b1=(64,), g_w2=(1 + A, 64), g_b2=(1 + A,),
                  g_attention_values=(B, A, 3), g_beta=(1,), g_alpha=(1,))
    fields = dict(n_scenes=B, points_per_scene=P, points=x, texels=texels, plane_res=res, texel_dtype=ops.TEXEL_F32,
                  texel_layout=ops.TEXELS_PLANAR, decoder_image=image, w1=w1.contiguous(), w2=w2.contiguous(), n_attention=A,
                  attention_values=att, use_sdf=1, beta=beta, alpha=alpha, scene_range=r, g_sigma=g_sig, g_rgb=g_rgb, scatter_mode=2)
    n_ws = _lib.struct_query('nfi_field_bwd_workspace_bytes', 'nfi_field_bwd_args', **fields)
    ws = torch.empty(((n_ws + 3) // 4,), dtype=torch.float32, device=dev)

    def call(bufs):
        with torch.cuda.device(dev):
            _lib.call_struct('nfi_field_query_bwd', 'nfi_field_bwd_args', ops._stream(x), workspace=ws, workspace_bytes=ws.numel() * 4,
                             **fields, **bufs)
    g = torch.Generator().manual_seed(1)
    prefill = {k: torch.randn(s, generator=g).to(dev) for k, s in shapes.items()}
    one = {k: torch.zeros(s, device=dev) for k, s in shapes.items()}
    call(one)
    assert all(float(v.abs().max()) > 0 for v in one.values())
    first = {k: v.clone() for k, v in prefill.items()}
    call(first)
    first_again = {k: v.clone() for k, v in prefill.items()}
    ws.fill_(float('nan'))                     # nothing of an earlier call may be read back: all scratch is rewritten
    call(first_again)
    twice = {k: v.clone() for k, v in first.items()}
    call(twice)
    for k in shapes:
        assert torch.equal(first[k], first_again[k]), k
        want = prefill[k].double() + 2 * one[k].double()
        err = float((twice[k].double() - want).abs().max() / want.abs().max())
        assert err <= 1e-6, (k, err)


# ------------------------------------------------------------------------------------------------
# 4. nfi_raygen_bwd_ordered
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['persp_white_fine_rand', 'persp_bbox_black_fine_rand', 'ortho_fine_det', 'center'])
@pytest.mark.parametrize('H,W', [(5, 7), (33, 65)])
def test_raygen_backward_ordered(gpu_device, name, H, W):
    """The cases of test_raygen_backward (perspective, bbox, orthographic) plus a principal-point offset, at its bound (2e-4
    of the gradient's maximum) against float64 autograd of the oracle; image sizes off the block size; six launches."""
    dev = gpu_device
    meta, t = load_golden('persp_white_fine_rand' if name == 'center' else name)
    B = meta['B']
    g = torch.Generator().manual_seed(3)
    w_o, w_d = torch.randn(B, H, W, 3, generator=g), torch.randn(B, H, W, 3, generator=g)
    center = (0.5 + 0.2 * (torch.rand(B, 2, generator=g) - 0.5)) if name == 'center' else None
    cam = t['cam2world'].double().requires_grad_()
    focal = t['focal'].double().requires_grad_() if 'focal' in t else None
    bbox = t['bbox'].double() if 'bbox' in t else None
    ro, rd = orc.ray_bundle(H, W, focal, cam, bbox, None if center is None else center.double())
    rd = orc.unit_dirs(rd)
    ref = torch.autograd.grad((ro * w_o.double()).sum() + (rd * w_d.double()).sum(), [cam] + ([focal] if focal is not None else []))
    dv = lambda x: None if x is None else x.to(dev)
    run = lambda ordered: ops.raygen_bwd(H, W, dv(t.get('focal')), t['cam2world'].to(dev), dv(t.get('bbox')), dv(center), True,
                                         w_o.view(-1, 3).to(dev), w_d.view(-1, 3).to(dev), ordered=ordered)
    g_cam, g_focal = run(True)
    rel_close(g_cam[:, :3], ref[0][:, :3], 'g_cam2world')
    if meta['ortho']:
        rel_close(g_cam, ref[0], 'g_cam2world incl. [3,3]')
    if focal is not None:
        rel_close(g_focal, ref[1], 'g_focal')
    # one rounding of the float64 sums: no farther from float64 than the kernel that rounds per block of 256 pixels
    old_cam, _ = run(False)
    scale = ref[0].abs().max()
    print('%s %dx%d: g_cam rel err ordered %.3e, per-block rounding %.3e' % (
        name, H, W, float((g_cam.double().cpu() - ref[0]).abs().max() / scale), float((old_cam.double().cpu() - ref[0]).abs().max() / scale)))
    for _ in range(5):
        again = run(True)
        assert torch.equal(again[0], g_cam) and (g_focal is None or torch.equal(again[1], g_focal))


# ------------------------------------------------------------------------------------------------
# 5. the whole render node
# ------------------------------------------------------------------------------------------------
def _render_case(dev, views, use_viewdir=False):
    torch.manual_seed(7)
    model = StandInGenerator(R_SCENE, attention_values=10, use_sdf=True, plane_res=32, use_viewdir=use_viewdir).to(dev)
    with torch.no_grad():
        model.alpha.fill_(0.2)
    nfi_gen.attach(model)
    g = torch.Generator().manual_seed(21)
    B, H, W, S = 2, 16, 16, 16
    d = types.SimpleNamespace(model=model, B=B, H=H, W=W, S=S, views=views)
    d.cam0 = look_at_cameras(B * views, 1.5, g)
    d.focal0 = torch.full((B * views,), 1.1)
    d.z = torch.randn(B, 512, generator=g).to(dev)
    d.w_rgb, d.w_mask = torch.randn(B * views, H, W, 3, generator=g), torch.randn(B * views, H, W, generator=g)
    d.cfg = types.SimpleNamespace(use_viewdir=use_viewdir, use_sdf=True, attention_values=10, fine_sampling=True)
    d.dcfg = {'scene_range': R_SCENE, 'white_background': True}
    return d


NAMES = ['w1', 'b1', 'w2', 'b2', 'beta', 'alpha', 'planes', 'attention_values', 'cam2world', 'focal']


def _render_grads(d, dev, deterministic, force=False, tap=None):
    """One forward + backward with fixed noise: rgb and the gradients of NAMES (the planes and the attention values are what
    the producer hands over: caught at the two modules' outputs)."""
    m = d.model
    render = nfi_render.make_render(d.cfg, d.dcfg, views_per_scene=d.views, deterministic_backward=deterministic)
    caught = {}
    hooks = [m.synthesis_network.register_forward_hook(lambda mod, i, o: caught.__setitem__('planes', o)),
             m.texture_mapper.register_forward_hook(lambda mod, i, o: caught.__setitem__('att', o))]
    cam, focal = d.cam0.to(dev).requires_grad_(), d.focal0.to(dev).requires_grad_()
    torch.manual_seed(33)
    try:
        rgb, depth, mask, _, _, _ = render(m, d.H, d.W, cam, focal, None, None, d.z, d.S, force_no_cam_grad=force)
    finally:
        for h in hooks:
            h.remove()
    loss = (rgb * d.w_rgb.to(dev)).sum() + (mask * d.w_mask.to(dev)).sum()
    leaves = [m.decoder.net[0].weight, m.decoder.net[0].bias, m.decoder.net[2].weight, m.decoder.net[2].bias, m.beta, m.alpha,
              caught['planes'], caught['att'], cam] + ([] if force else [focal])
    return rgb.detach(), torch.autograd.grad(loss, leaves)


@pytest.mark.parametrize('views,force', [(1, False), (2, False), (1, True)])
def test_render_with_deterministic_backward_repeats_bit_for_bit(gpu_device, views, force):
    dev = gpu_device
    d = _render_case(dev, views)
    rgb, first = _render_grads(d, dev, True, force)
    assert all(float(t.abs().max()) > 0 for t in first)
    for _ in range(3):
        rgb_again, again = _render_grads(d, dev, True, force)
        assert torch.equal(rgb_again, rgb)
        for n, a, b in zip(NAMES, again, first):
            assert torch.equal(a, b), n
    # the option is the backward's: the forward is the default option's, bit for bit
    rgb_default, default = _render_grads(d, dev, False, force)
    assert torch.equal(rgb_default, rgb)
    for n, a, b in zip(NAMES, first, default):
        print('views %d force %s: grad %-18s ordered vs default rel %.3e' % (
            views, force, n, float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))))


def test_render_with_deterministic_backward_against_the_oracle(gpu_device):
    """The bounds of test_render_backward_end_to_end: 2e-3 of the gradient's maximum, or four times what float32 rounding
    alone moves the oracle's gradient."""
    from test_host_api_gpu import RandTap
    dev = gpu_device
    d = _render_case(dev, 1)
    with RandTap() as tap:
        rgb, got = _render_grads(d, dev, True)

    def oracle_grads(dtype):
        ref_model = copy.deepcopy(d.model).cpu().to(dtype)
        planes, att = ref_model.planes_and_values(d.z.cpu().to(dtype))
        dec = ref_model.decoder.net
        ocam, ofocal = d.cam0.to(dtype).requires_grad_(), d.focal0.to(dtype).requires_grad_()
        draws = [t.to(dtype) for t in tap.draws]
        o = orc.render(planes, dec[0].weight, dec[0].bias, dec[2].weight, dec[2].bias, ocam, ofocal, d.H, d.W, d.S, R_SCENE,
                       white_background=True, fine_sampling=True, noise_coarse=draws[0], noise_fine=draws[1], use_sdf=True,
                       beta=ref_model.beta, alpha=ref_model.alpha, attention_values=att)
        oloss = (o['rgb'] * d.w_rgb.to(dtype)).sum() + (o['mask'] * d.w_mask.to(dtype)).sum()
        return o, torch.autograd.grad(oloss, [dec[0].weight, dec[0].bias, dec[2].weight, dec[2].bias, ref_model.beta,
                                              ref_model.alpha, planes, att, ocam, ofocal])
    o, ref = oracle_grads(torch.float64)
    _, ref32 = oracle_grads(torch.float32)
    rel_close(rgb, o['rgb'], 'forward rgb', 2e-4)
    for n, a, b, b32 in zip(NAMES, got, ref, ref32):
        if n == 'cam2world':
            a, b, b32 = a[:, :3], b[:, :3], b32[:, :3]
        if n == 'planes':
            a = a.view(b.shape)
        scale = b.abs().max().clamp_min(1e-12)
        noise = float((b32.double() - b).abs().max() / scale)
        print('grad %-18s rel %.3e (float32 oracle %.3e)' % (n, float((a.double().cpu() - b).abs().max() / scale), noise))
        rel_close(a, b, 'grad ' + n, max(2e-3, 4 * noise))


def test_render_with_deterministic_backward_refuses_the_viewdir_decoder(gpu_device):
    dev = gpu_device
    d = _render_case(dev, 1, use_viewdir=True)
    render = nfi_render.make_render(d.cfg, d.dcfg, deterministic_backward=True)
    cam, focal = d.cam0.to(dev).requires_grad_(), d.focal0.to(dev)
    with pytest.raises(NotImplementedError, match='deterministic_backward'):
        render(d.model, d.H, d.W, cam, focal, None, None, d.z, d.S)
    with torch.no_grad():                      # inference ignores the option
        rgb = render(d.model, d.H, d.W, cam.detach(), focal, None, None, d.z, d.S)[0]
    assert rgb.shape == (d.B, d.H, d.W, 3)
