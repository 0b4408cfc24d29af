"""GPU checks of the order of a field turn (nfi_device.hpp, field_wave's plain loop and tile_mlp<N, 1>): both tiles'
gather operands are fetched at the top of the turn, tile a's L -> M transpose runs behind tile b's load issue, and the
decoder's operands are read one MFMA group ahead, the first group together with the last transpose read.  No arithmetic
changed, so everything here holds for the schedule before it as well; the cases are the ones where the new order has an
edge:

  * 1, 2, 3 and 4 live tiles per pass (the unpaired last turn with the deferred transpose), and live tiles with a gap
    (tile 0 and tile 3 only: a coarse noise that throws samples 16 .. 47 far behind the cube);
  * S = 16 (one tile), 40 (ragged last tile) and 64; fine pass on and off; A = 10 and A = 0; fp32, fp16 and bf16 texels;
    tuning 0 (split-fp16 decoder) and 8 (exact fp32: the same turn around the other decoder);
  * a second scene marched by the same waves right behind the first (`stage` and the decoder's operand registers across a
    scene change), bit for bit the scene rendered alone;
  * the field query (the sampler closure shares the turn), both decoders, at 1, 17 and 65 points.

Images are 16 x 16 and 24 x 24 with two scenes; the scene-change case alone needs more rays than the chip holds waves and
takes the 64 x 64 of tests/test_field_epilogue_gpu.py, whose scenes and workspace helpers are used throughout.
Tolerances are those of tests/test_field_epilogue_gpu.py and tests/test_hip_parity.py for the same quantities."""
import pytest
import torch

from nerf_from_image_amd import ops
from oracle import nfi_oracle as orc
from parity_util import hip_render
from stand_in import look_at_cameras
from test_field_epilogue_gpu import (FAR_OFFSET, HIT_OFFSET, NEAR_OFFSET, R, TILE_RANGES, live_tile_masks, push_planes,
                                     render_case, smooth_scene, staged_setup)
from test_hip_parity import ATOL, close, exact, sigma_close

pytestmark = pytest.mark.gpu

TEXELS = {'fp32': (ops.TEXEL_F32, None, ATOL), 'fp16': (ops.TEXEL_F16, torch.float16, 2e-4),
          'bf16': (ops.TEXEL_BF16, torch.bfloat16, 2e-4)}
# (side, S, fine, A, texels, tuning): every value of every axis, and the pairs that share code (16-bit texels at three
# workgroups per CU with and without the fine pass, A = 0 with either decoder; the exact decoder exists for fp32 texels)
RENDER_CASES = [(16, 64, True, 10, 'fp32', 0), (24, 64, True, 10, 'fp32', 0), (24, 40, True, 10, 'fp32', 0),
                (16, 16, True, 10, 'fp32', 0), (16, 40, False, 10, 'fp32', 0), (24, 64, False, 0, 'fp32', 0),
                (24, 40, True, 0, 'fp32', 8), (16, 64, True, 10, 'fp32', 8), (16, 16, False, 10, 'fp32', 8),
                (24, 64, True, 10, 'fp16', 0), (16, 40, False, 10, 'fp16', 0), (24, 16, True, 0, 'bf16', 0),
                (16, 64, True, 10, 'bf16', 0), (24, 40, True, 10, 'fp16', 0)]


@pytest.mark.parametrize('side,S,fine,A,tex,tuning', RENDER_CASES,
                         ids=['%dx%d_S%d_%s_A%d_%s_t%d' % (c[0], c[0], c[1], 'fine' if c[2] else 'coarse', c[3], c[4], c[5])
                              for c in RENDER_CASES])
def test_fused_render_against_oracle(gpu_device, side, S, fine, A, tex, tuning):
    """pixels against the CPU oracle; the rays that meet the cube bit for bit with and without the miss runs skipped"""
    dev = gpu_device
    texel_dtype, rounded, tol = TEXELS[tex]
    meta, t, o = render_case(side, side, S, fine, A=A, rounded=rounded)
    assert float(o['mask'].max()) > 0.1, 'scene should not be empty'
    skip = hip_render(meta, t, dev, skip_missed_rays=True, texel_dtype=texel_dtype, tuning=tuning)
    march = hip_render(meta, t, dev, skip_missed_rays=False, texel_dtype=texel_dtype, tuning=tuning)
    n = meta['B'] * side * side
    ws = ops.render_setup(t['cam2world'].to(dev), t['focal'].to(dev), side, side, R)
    hits = ((ws[HIT_OFFSET(n):HIT_OFFSET(n) + n] & 2) != 0).view(meta['B'], side, side)
    assert 0 < int(hits.sum()), 'some ray should meet the cube'
    for k in ('rgb', 'depth', 'mask'):
        close(skip[k], o[k], tol, k)
        close(march[k], o[k], tol, k + ', every ray marched')
        exact(skip[k][hits], march[k][hits], 'skip_missed_rays on / off on the rays that hit, ' + k)


def staged_pixels(ws, n, B, H, W, S, field, taps):
    """field query + composite on the fused launch's own depths, with the fused kernel's decoder arithmetic"""
    ro = ws[576:576 + 12 * n].view(torch.float32).view(n, 3)
    rd = ws[576 + 12 * n:576 + 24 * n].view(torch.float32).view(n, 3)
    tc, tf = taps['t_coarse'].reshape(n, S), taps['t_fine'].reshape(n, S)
    q = {}
    for name, dep in (('c', tc), ('f', tf)):
        pts = ops.points_on_rays(ro, rd, dep)
        q[name] = ops.field_query(pts.view(B, H * W * S, 3), *field, mlp_precision=1)
    rgb, depth, mask, _, _ = ops.composite(rd, tc, q['c']['sigma'].view(n, S), q['c']['rgb'].view(n, S, 3), tf,
                                           q['f']['sigma'].view(n, S), q['f']['rgb'].view(n, S, 3), white_background=True)
    return dict(rgb=rgb.view(n, 3), depth=depth.view(n), mask=mask.view(n))


@pytest.mark.parametrize('side', [16, 24])
def test_one_to_four_live_tiles_against_staged_path(gpu_device, side):
    """near / far of chosen rays moved so that 1, 2, 3 or all 4 tiles of the coarse pass are live, at either end of the pass:
    every pairing of a turn, the unpaired last turn after a paired one (3 tiles) and alone (1 tile)"""
    dev = gpu_device
    B, H, W, S = 2, side, side, 64
    n = B * H * W
    cam, focal, field, render = staged_setup(dev, B, H, W, S, 4242 + side)
    ws = ops.render_setup(cam, focal, H, W, R)
    assert bool(((ws[HIT_OFFSET(n):HIT_OFFSET(n) + n] & 2) != 0).all()), 'the cameras of this test leave no ray outside the cube'
    push_planes(ws, n, [r for r in range(n) if r % 6 != 5], TILE_RANGES)
    out = render(ws.clone(), skip_missed_rays=True)
    taps = render(ws.clone(), skip_missed_rays=True, taps=('t_coarse', 't_fine'))
    masks = live_tile_masks(ws, n, taps['t_coarse'])
    for want in (0b0110, 0b0010, 0b0100, 0b0111, 0b1110, 0b1111):
        assert int((masks == want).sum()) >= 1, ('no ray with live-tile mask', bin(want), masks.tolist())
    ref = staged_pixels(ws, n, B, H, W, S, field, taps)
    assert float(ref['mask'].max()) > 0.1, 'scene should not be empty'
    for k in ('rgb', 'depth', 'mask'):
        close(out[k].view(ref[k].shape), ref[k], 1e-5, 'fused vs staged ' + k)
    full = render(ws.clone(), skip_missed_rays=False)
    for k in ('rgb', 'depth', 'mask'):
        exact(full[k], out[k], 'skip_missed_rays=False, ' + k)


@pytest.mark.parametrize('tuning', [0, 8], ids=['split_fp16', 'exact_fp32'])
def test_live_tiles_with_a_gap(gpu_device, tuning):
    """Coarse noise of 1000 steps on samples 16 .. 47 of every other ray: they land far behind the cube, tiles 1 and 2 are
    dead, tiles 0 and 3 live - one paired turn whose tiles are not neighbours.  The per-sample taps of the fused launch
    against the field query on the same points (the taps kernels share field_wave), and the plain launch's pixels with and
    without the miss runs skipped."""
    dev = gpu_device
    B, H, W, S, A = 2, 16, 16, 64, 10
    n = B * H * W
    t, g = smooth_scene(B, A, 16, 9100 + tuning)
    cam = look_at_cameras(B, 6.0, g).to(dev)
    focal = torch.full((B,), 16.0, device=dev)           # a long lens from far away: every ray crosses the cube
    mv = lambda v: v.to(dev)
    texels = ops.planes_to_texels(mv(t['planes']))
    image = ops.decoder_pack(mv(t['w1']), mv(t['b1']), mv(t['w2']), mv(t['b2']), A)
    field = (texels, image, R, A, mv(t['attention_values']), True, mv(t['beta']), mv(t['alpha']))
    noise_c = torch.rand(B, H, W, S, generator=g)
    noise_c.view(n, S)[::2, 16:48] += 1000.0
    noise_c, noise_f = noise_c.to(dev), torch.rand(n, S, generator=g).to(dev)
    ws = ops.render_setup(cam, focal, H, W, R)

    def render(**kw):
        return ops.render_fwd(cam, focal, H, W, S, *field, noise_coarse=noise_c, noise_fine=noise_f, fine_sampling=True,
                              white_background=True, workspace=ws.clone(), rays_ready=True, tuning=tuning, **kw)
    taps = render(skip_missed_rays=True, taps=('t_coarse', 'sigma_coarse', 'rgb_coarse', 't_fine', 'sigma_fine', 'rgb_fine'))
    masks = live_tile_masks(ws, n, taps['t_coarse'])
    assert bool((masks[::2] == 0b1001).all()) and int((masks[1::2] == 0b1111).sum()) >= 1, masks.tolist()
    ro = ws[576:576 + 12 * n].view(torch.float32).view(n, 3)
    rd = ws[576 + 12 * n:576 + 24 * n].view(torch.float32).view(n, 3)
    for name in ('coarse', 'fine'):
        dep = taps['t_' + name].reshape(n, S)
        pts = ops.points_on_rays(ro, rd, dep)
        q = ops.field_query(pts.view(B, H * W * S, 3), *field, want_outside=True, mlp_precision=0 if tuning == 8 else 1)
        inside = q['outside'].view(n, S) == 0
        sigma, rgb = taps['sigma_' + name].reshape(n, S), taps['rgb_' + name].reshape(n, S, 3)
        assert int(inside.sum()) > n * S // 4
        assert float(sigma[~inside].abs().max()) == 0.0, name + ': a sample outside the cube has no density'
        sigma_close(sigma[inside], q['sigma'].view(n, S)[inside], name + ' sigma of the samples inside')
        close(rgb[inside], q['rgb'].view(n, S, 3)[inside], 1e-5, name + ' rgb of the samples inside')
    skip, march = render(skip_missed_rays=True), render(skip_missed_rays=False)
    for k in ('rgb', 'depth', 'mask'):
        assert bool(torch.isfinite(skip[k]).all()), k
        exact(skip[k], march[k], 'skip_missed_rays on / off, ' + k)
    assert float(skip['mask'].max()) > 0.1, 'scene should not be empty'


@pytest.mark.parametrize('tuning', [0, 8], ids=['split_fp16', 'exact_fp32'])
def test_second_scene_behind_the_first(gpu_device, tuning):
    """more rays than the chip holds waves: a wave marches rays of scene 0 and then of scene 1, some of them with skipped
    tiles and unpaired turns; scene 1's pixels are bit for bit those of the scene rendered alone"""
    dev = gpu_device
    B, H, W, S = 2, 64, 64, 64
    n1 = H * W
    cam, focal, field, render = staged_setup(dev, B, H, W, S, 778)
    edited = [r for r in range(n1) if r % 3 != 2]
    ws = ops.render_setup(cam, focal, H, W, R)
    push_planes(ws, B * n1, [n1 + r for r in edited], TILE_RANGES)
    ws1 = ops.render_setup(cam[1:2], focal[1:2], H, W, R)
    push_planes(ws1, n1, edited, TILE_RANGES)
    n = B * n1
    assert torch.equal(ws[NEAR_OFFSET(n) + 4 * n1:NEAR_OFFSET(n) + 4 * n], ws1[NEAR_OFFSET(n1):NEAR_OFFSET(n1) + 4 * n1])
    assert torch.equal(ws[FAR_OFFSET(n) + 4 * n1:FAR_OFFSET(n) + 4 * n], ws1[FAR_OFFSET(n1):FAR_OFFSET(n1) + 4 * n1])
    both = render(ws.clone(), skip_missed_rays=True, tuning=tuning)
    alone = render(ws1.clone(), slice(1, 2), skip_missed_rays=True, tuning=tuning)
    for k in ('rgb', 'depth', 'mask'):
        assert bool(torch.isfinite(both[k]).all()), k
        exact(both[k][1], alone[k][0], 'scene 1 behind scene 0, ' + k)
    assert float(alone['mask'].max()) > 0.1, 'scene should not be empty'


@pytest.mark.parametrize('A', [10, 0])
def test_field_query_shares_the_turn(gpu_device, A):
    """the sampler closure at 1 point (one unpaired turn), 17 (a pair, the second tile with one point) and 65 (a second
    call of the wave), both decoders, against the CPU oracle"""
    dev = gpu_device
    B = 2
    t, g = smooth_scene(B, A, 16, 9300 + A)
    att = t.get('attention_values')
    texels = ops.planes_to_texels(t['planes'].to(dev))
    image = ops.decoder_pack(t['w1'].to(dev), t['b1'].to(dev), t['w2'].to(dev), t['b2'].to(dev), A)
    for P in (1, 17, 65):
        x = (torch.rand(B, P, 3, generator=g) * 2 - 1) * R * 1.3
        ref = orc.field_query(t['planes'], t['w1'], t['b1'], t['w2'], t['b2'], x, R, True, t['beta'], t['alpha'], att)
        for prec in (0, 1):
            what = 'A %d, P %d, mlp_precision %d' % (A, P, prec)
            q = ops.field_query(x.to(dev), texels, image, R, A, None if att is None else att.to(dev), True,
                                t['beta'].to(dev), t['alpha'].to(dev), want_sdf=True, want_semantics=A > 0, want_outside=True,
                                mlp_precision=prec)
            exact(q['outside'].float(), ref['outside'], what + ': outside')
            close(q['sdf'], ref['sdf'], 1e-5, what + ': sdf')
            sigma_close(q['sigma'], ref['sigma'], what + ': sigma')
            close(q['rgb'], ref['rgb'], ATOL, what + ': rgb')
            if A > 0:
                close(q['semantics'], ref['semantics'], 1e-5, what + ': semantics')
