"""GPU checks of the field decoder's epilogue in the sample layout (nfi_device.hpp: field_wave parks every live tile's
decoder outputs in a per-wave LDS table and runs sample_epilogue once per call, lane = sample) - the plain render kernels
with attention - and, on the same cases, of the per-tile epilogue every other kernel keeps.

  * the field query against the CPU oracle over point counts that give one tile, an unpaired third tile, a partial last
    chunk and a second chunk per wave, and attention sizes that end at / one past every channel group's boundary;
  * the fused render against the oracle and against itself: one to four tiles per pass, the wide and the single-pass
    kernel, the extra maps, 16-bit texels, the training stash;
  * skipped tiles: the ray set-up runs alone (ops.render_setup), `near` / `far` of chosen rays are moved in the workspace
    (floats at byte 576 + 24 n and 576 + 28 n of the documented prefix) so that whole 16-sample tiles fall outside the
    cube, and the kernel is launched on that workspace (rays_ready=True);
  * stale table slots: a skipped tile's slots keep what an earlier ray - of another scene - left there.

Tolerances are the ones tests/test_hip_parity.py and tests/test_kernel_matrix.py use for the same quantities."""
import pytest
import torch

from nerf_from_image_amd import ops
from oracle import nfi_oracle as orc
from parity_util import err, hip_render, oracle_normal_map, oracle_render
from stand_in import look_at_cameras
from test_hip_parity import ATOL, close, exact, sigma_close

pytestmark = pytest.mark.gpu
R = 0.55
POINTS = (1, 15, 16, 17, 33, 48, 64, 65, 130)
ATTENTION = (0, 1, 3, 4, 7, 8, 11, 12, 14)
NEAR_OFFSET = lambda n: 576 + 24 * n
FAR_OFFSET = lambda n: 576 + 28 * n
HIT_OFFSET = lambda n: 576 + 32 * n


def smooth_scene(B, A, PR, seed):
    """a band-limited random field (low-resolution noise interpolated, a little white noise on top) and a random decoder, its
    distance bias shifted so that the zero level set runs through the cube (half of 512 random points inside the surface)"""
    g = torch.Generator().manual_seed(seed)
    n_out = 1 + A if A > 0 else 4
    low = torch.randn(B * 3, 32, 6, 6, generator=g)
    planes = torch.nn.functional.interpolate(low, size=(PR, PR), mode='bilinear', align_corners=True).view(B, 3, 32, PR, PR) \
        + 0.1 * torch.randn(B, 3, 32, PR, PR, generator=g)
    t = dict(planes=planes, w1=torch.randn(64, 32, generator=g), b1=0.3 * torch.randn(64, generator=g),
             w2=torch.randn(n_out, 64, generator=g), b2=0.3 * torch.randn(n_out, generator=g),
             beta=torch.tensor([0.12]), alpha=torch.tensor([0.3]))
    if A > 0:
        t['attention_values'] = torch.rand(B, A, 3, generator=g) * 2 - 1          # (different rows per scene)
    x = (torch.rand(B, 512, 3, generator=g) * 2 - 1) * R
    sdf = orc.field_query(planes, t['w1'], t['b1'], t['w2'], t['b2'], x, R, True, t['beta'], t['alpha'], t.get('attention_values'))['sdf']
    t['b2'][0] -= sdf.median()
    return t, g


# ---------------------------------------------------------------------------------------------------------------------
# field query against the CPU oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('use_sdf', [True, False], ids=['sdf', 'density'])
@pytest.mark.parametrize('A', ATTENTION)
def test_field_query_against_oracle(gpu_device, A, use_sdf):
    dev = gpu_device
    for B in (1, 2):
        t, g = smooth_scene(B, A, 16, 9000 + 31 * A + B)
        att = t.get('attention_values')
        texels = ops.planes_to_texels(t['planes'].to(dev))
        image = ops.decoder_pack(t['w1'].to(dev), t['b1'].to(dev), t['w2'].to(dev), t['b2'].to(dev), A)
        for P in POINTS:
            x = (torch.rand(B, P, 3, generator=g) * 2 - 1) * R * 1.3
            # outside the cube, far outside, on its faces and in a corner (where the point count leaves room)
            special = torch.tensor([[R, -R, R], [R, 0.0, 0.0], [-R, -R, -R], [2 * R, 0.1, 0.1], [1e6, -1e6, 3.0], [0.0, 0.0, -R]])
            k = min(P - 1, len(special)) if P > 1 else (1 if B == 2 else 0)
            x[-1, P - k:] = special[:k]
            ref = orc.field_query(t['planes'], t['w1'], t['b1'], t['w2'], t['b2'], x, R, use_sdf, t['beta'], t['alpha'], att)
            for prec in (0, 1):
                what = 'A %d, B %d, P %d, mlp_precision %d' % (A, B, P, prec)
                q = ops.field_query(x.to(dev), texels, image, R, A, None if att is None else att.to(dev), use_sdf,
                                    t['beta'].to(dev), t['alpha'].to(dev), want_sdf=True, want_semantics=A > 0, want_outside=True,
                                    mlp_precision=prec)
                exact(q['outside'].float(), ref['outside'], what + ': outside')
                close(q['sdf'], ref['sdf'], 1e-5, what + ': sdf')
                sigma_close(q['sigma'], ref['sigma'], what + ': sigma')
                close(q['rgb'], ref['rgb'], ATOL, what + ': rgb')
                if A > 0:
                    close(q['semantics'], ref['semantics'], 1e-5, what + ': semantics')


# ---------------------------------------------------------------------------------------------------------------------
# fused render against the oracle and against itself
# ---------------------------------------------------------------------------------------------------------------------
_cases = {}


def render_case(H, W, S, fine, A=10, rounded=None):
    """(meta, tensors, oracle render) in the golden cases' form: made once per shape, never written"""
    key = (H, W, S, fine, A, rounded)
    if key not in _cases:
        B = 2
        t, g = smooth_scene(B, A, 16, 7000 + 131 * H + 7 * S + (1 if fine else 0))
        if rounded is not None:
            t['planes'] = t['planes'].to(rounded).float()
        t['cam2world'] = look_at_cameras(B, 1.7, g)
        t['focal'] = torch.full((B,), 1.6)          # wide enough for rays along the border to miss or graze the cube
        t['noise_coarse'] = torch.rand(B, H, W, S, generator=g)
        if fine:
            t['noise_fine'] = torch.rand(B * H * W, S, generator=g)
        meta = dict(B=B, H=H, W=W, S=S, A=A, scene_range=R, white=True, fine=fine, sdf=True)
        _cases[key] = (meta, t, oracle_render(meta, t, 'cpu'))
    return _cases[key]


def coords_map(o):
    t_sorted = o['t_sorted'] if 't_sorted' in o else o['t_coarse']          # (a single pass is composited in the order given)
    pts = o['ro'].unsqueeze(-2) + o['rd'].unsqueeze(-2) * t_sorted.unsqueeze(-1)
    return (o['weights'].unsqueeze(-1) * pts).sum(-2)


@pytest.mark.parametrize('fine', [True, False], ids=['fine', 'coarse_only'])
@pytest.mark.parametrize('S', [8, 16, 24, 40, 64, 128])
@pytest.mark.parametrize('H,W', [(8, 8), (12, 20)])
def test_fused_render_and_maps(gpu_device, H, W, S, fine):
    """one to four tiles per pass (S <= 64), the wide kernel (S = 128): pixels and the semantics / coords / normals maps"""
    meta, t, o = render_case(H, W, S, fine)
    plain = hip_render(meta, t, gpu_device, skip_missed_rays=True)
    assert float(o['mask'].max()) > 0.1, 'scene should not be empty'
    for k in ('rgb', 'depth', 'mask'):
        close(plain[k], o[k], ATOL, k)
    full = hip_render(meta, t, gpu_device, skip_missed_rays=False)
    for k in ('rgb', 'depth', 'mask'):
        exact(full[k], plain[k], 'skip_missed_rays=False, ' + k)
    m = hip_render(meta, t, gpu_device, skip_missed_rays=True, want_semantics=True, want_coords=True)
    for k in ('rgb', 'depth', 'mask'):
        exact(m[k], plain[k], 'extra-maps launch, ' + k)
    close(m['semantics'], o['semantics'], 1e-5, 'semantic map')
    close(m['coords'], coords_map(o), 1e-5, 'coords map')
    n = hip_render(meta, t, gpu_device, skip_missed_rays=True, want_normals=True, want_semantics=True, want_coords=True)
    for k in ('rgb', 'depth', 'mask'):
        exact(n[k], plain[k], 'normal-map launch, ' + k)
    close(n['semantics'], o['semantics'], 1e-5, 'semantic map next to the normals')
    close(n['normals'], oracle_normal_map(meta, t, o), 3e-5, 'normal map')


@pytest.mark.parametrize('H,W', [(8, 8), (12, 20)])
def test_fused_render_long_kernel(gpu_device, H, W):
    """the single-pass kernel at its smallest S (129)"""
    meta, t, o = render_case(H, W, 129, False)
    plain = hip_render(meta, t, gpu_device, skip_missed_rays=True)
    for k in ('rgb', 'depth', 'mask'):
        close(plain[k], o[k], ATOL, k)


@pytest.mark.parametrize('S', [24, 64, 128])
@pytest.mark.parametrize('tex,torch_dtype', [(ops.TEXEL_BF16, torch.bfloat16), (ops.TEXEL_F16, torch.float16)], ids=['bf16', 'fp16'])
def test_fused_render_16bit_texels(gpu_device, tex, torch_dtype, S):
    """16-bit texel storage (three workgroups per CU for S <= 64) against the oracle on the same rounded planes"""
    meta, t, o = render_case(12, 20, S, True, rounded=torch_dtype)
    r = hip_render(meta, t, gpu_device, skip_missed_rays=True, texel_dtype=tex)
    for k in ('rgb', 'depth', 'mask'):
        close(r[k], o[k], 2e-4, k)


@pytest.mark.parametrize('S', [24, 64, 128])
def test_fused_render_training_stash(gpu_device, S):
    """the training-stash launch: its pixels are the plain launch's, its rows the per-sample taps of a launch that skips nothing"""
    meta, t, o = render_case(12, 20, S, True)
    st = hip_render(meta, t, gpu_device, skip_missed_rays=True, stash=True, taps=('hit',))
    full = hip_render(meta, t, gpu_device, taps=('t_coarse', 'sigma_coarse', 'rgb_coarse', 't_fine', 'sigma_fine', 'rgb_fine'))
    for k in ('rgb', 'depth', 'mask'):
        close(st[k], o[k], ATOL, 'stash launch, ' + k)
    hit = (st['hit'] & 2) != 0
    for k, (a, b) in dict(stash_t=('t_coarse', 't_fine'), stash_sigma=('sigma_coarse', 'sigma_fine'),
                          stash_rgb=('rgb_coarse', 'rgb_fine')).items():
        assert torch.equal(st[k][:, :, :, :S][hit], full[a][hit]), k
        assert torch.equal(st[k][:, :, :, S:][hit], full[b][hit]), k


# ---------------------------------------------------------------------------------------------------------------------
# skipped tiles and stale table slots
# ---------------------------------------------------------------------------------------------------------------------
# live tiles [k0, k1) of the four 16-sample tiles of a 64-sample coarse pass: masks 0110, 0100, 0010, 0111, 1110
TILE_RANGES = ((1, 3), (1, 2), (2, 3), (0, 3), (1, 4))


def push_planes(ws, n, rays, ranges):
    """moves near back and far forward for `rays` (cycling through `ranges`) so that the cube's span [near, far] of the ray
    covers tiles [k0, k1) of the pass and nothing else; returns nothing, edits the workspace"""
    near = ws[NEAR_OFFSET(n):NEAR_OFFSET(n) + 4 * n].view(torch.float32)
    far = ws[FAR_OFFSET(n):FAR_OFFSET(n) + 4 * n].view(torch.float32)
    for i, ray in enumerate(rays):
        k0, k1 = ranges[i % len(ranges)]
        a, b = float(near[ray]), float(far[ray])
        delta = 0.02 * (b - a)
        q = (b - a + 2 * delta) / (k1 - k0)
        lo = a - delta - k0 * q
        assert lo > 0.1, 'the edited near plane must stay in front of the clamp of the ray set-up'
        near[ray] = lo
        far[ray] = lo + 4 * q


def live_tile_masks(ws, n, t_coarse):
    """4-bit mask per ray, bit k: tile k of the coarse pass has a sample inside the cube (what field_wave's ballot sees)"""
    ro = ws[576:576 + 12 * n].view(torch.float32).view(n, 3)
    rd = ws[576 + 12 * n:576 + 24 * n].view(torch.float32).view(n, 3)
    pts = ro[:, None, :] + rd[:, None, :] * t_coarse.reshape(n, -1, 1)
    inside = ((pts / R).abs() <= 1.0).all(-1).view(n, 4, 16).any(-1)
    return (inside.int() * torch.tensor([1, 2, 4, 8], device=inside.device)).sum(-1)


def staged_setup(dev, B, H, W, S, seed, planes_edit=None):
    t, g = smooth_scene(B, 10, 16, seed)
    if planes_edit is not None:
        planes_edit(t['planes'])
    cam = look_at_cameras(B, 6.0, g).to(dev)
    focal = torch.full((B,), 16.0, device=dev)           # a long lens from far away: every ray crosses the cube
    mv = lambda v: v.to(dev)
    texels = ops.planes_to_texels(mv(t['planes']))
    image = ops.decoder_pack(mv(t['w1']), mv(t['b1']), mv(t['w2']), mv(t['b2']), 10)
    noise_c = torch.rand(B, H, W, S, generator=g).to(dev)
    noise_f = torch.rand(B * H * W, S, generator=g).to(dev)
    field = (texels, image, R, 10, mv(t['attention_values']), True, mv(t['beta']), mv(t['alpha']))

    def render(ws, sel=slice(None), **kw):
        nb = cam[sel].shape[0]
        return ops.render_fwd(cam[sel], focal[sel], H, W, S, texels[sel], image, R, 10, field[4][sel], True, field[6], field[7],
                              noise_coarse=noise_c[sel], noise_fine=noise_f.view(B, -1, S)[sel].reshape(nb * H * W, S),
                              fine_sampling=True, white_background=True, workspace=ws, rays_ready=True, **kw)
    return cam, focal, field, render


def test_skipped_tiles_against_staged_path(gpu_device):
    """whole tiles outside the cube at the front, the back or both ends of the coarse pass: the fused launch against the field
    query + composite on the same depths, and against the same launch with skip_missed_rays=False"""
    dev = gpu_device
    B, H, W, S = 2, 8, 8, 64
    n = B * H * W
    cam, focal, field, render = staged_setup(dev, B, H, W, S, 4242)
    ws = ops.render_setup(cam, focal, H, W, R)
    assert bool(((ws[HIT_OFFSET(n):HIT_OFFSET(n) + n] & 2) != 0).all()), 'the cameras of this test leave no ray outside the cube'
    push_planes(ws, n, [r for r in range(n) if r % 6 != 5], TILE_RANGES)
    out = render(ws.clone(), skip_missed_rays=True)
    taps = render(ws.clone(), skip_missed_rays=True, taps=('t_coarse', 't_fine'))
    masks = live_tile_masks(ws, n, taps['t_coarse'])
    for want in (0b0110, 0b0010, 0b0100, 0b0111, 0b1110, 0b1111):
        assert int((masks == want).sum()) >= 1, ('no ray with live-tile mask', bin(want), masks.tolist())
    # the staged path on the same depths, with the fused kernel's decoder arithmetic
    ro = ws[576:576 + 12 * n].view(torch.float32).view(n, 3)
    rd = ws[576 + 12 * n:576 + 24 * n].view(torch.float32).view(n, 3)
    tc, tf = taps['t_coarse'].reshape(n, S), taps['t_fine'].reshape(n, S)
    q = {}
    for name, dep in (('c', tc), ('f', tf)):
        pts = ops.points_on_rays(ro, rd, dep)
        q[name] = ops.field_query(pts.view(B, H * W * S, 3), *field, mlp_precision=1)
    rgb, depth, mask, _, _ = ops.composite(rd, tc, q['c']['sigma'].view(n, S), q['c']['rgb'].view(n, S, 3), tf,
                                           q['f']['sigma'].view(n, S), q['f']['rgb'].view(n, S, 3), white_background=True)
    assert float(mask.max()) > 0.1, 'scene should not be empty'
    close(out['rgb'].view(n, 3), rgb.view(n, 3), 1e-5, 'fused vs staged rgb')
    close(out['depth'].view(n), depth.view(n), 1e-5, 'fused vs staged depth')
    close(out['mask'].view(n), mask.view(n), 1e-5, 'fused vs staged mask')
    full = render(ws.clone(), skip_missed_rays=False)
    for k in ('rgb', 'depth', 'mask'):
        exact(full[k], out[k], 'skip_missed_rays=False, ' + k)


@pytest.mark.parametrize('tuning', [0, 8], ids=['split_fp16', 'exact_fp32'])
def test_stale_table_slots_of_another_scene(gpu_device, tuning):
    """Scene 0's planes hold inf around one cube corner; scene 1, marched behind it by the same waves, has rays with skipped
    tiles, whose table slots keep what scene 0's rays left there.  Its pixels are finite and bit for bit those of the scene
    rendered alone: a skipped tile's slots are never read into a result.
    The poison has to REACH the table for that to say anything.  In the split-fp16 kernel it does not: the hidden layer's
    softplus is a v_med3 against 128, which returns 128 for a NaN unit, and scene 0 renders finite pixels.  With tuning
    bit 3 (NFI_TUNING_EXACT_FP32_MLP: the plain kernel with the exact-fp32 decoder, the same field_wave and epilogue) NaN
    goes through to the decoder's outputs - asserted on scene 0's pixels - so that an epilogue which zeroed by
    multiplication, or took a wrong live bit, would put NaN into scene 1."""
    dev = gpu_device
    B, H, W, S = 2, 64, 64, 64               # more rays than the chip holds waves: a wave marches rays of both scenes
    n1 = H * W

    def poison(planes):
        planes[0, :, :, :8, :8] = float('inf')
    cam, focal, field, render = staged_setup(dev, B, H, W, S, 777, planes_edit=poison)
    edited = [r for r in range(n1) if r % 3 != 2]
    ws = ops.render_setup(cam, focal, H, W, R)
    push_planes(ws, B * n1, [n1 + r for r in edited], TILE_RANGES)
    ws1 = ops.render_setup(cam[1:2], focal[1:2], H, W, R)
    push_planes(ws1, n1, edited, TILE_RANGES)
    n = B * n1
    assert torch.equal(ws[NEAR_OFFSET(n) + 4 * n1:NEAR_OFFSET(n) + 4 * n], ws1[NEAR_OFFSET(n1):NEAR_OFFSET(n1) + 4 * n1])
    assert torch.equal(ws[FAR_OFFSET(n) + 4 * n1:FAR_OFFSET(n) + 4 * n], ws1[FAR_OFFSET(n1):FAR_OFFSET(n1) + 4 * n1])
    taps = render(ws1.clone(), slice(1, 2), skip_missed_rays=True, taps=('t_coarse',))
    masks = live_tile_masks(ws1, n1, taps['t_coarse'])
    assert int(((masks != 0b1111) & (masks != 0)).sum()) >= 1, 'at least one ray of scene 1 has a skipped tile'
    both = render(ws.clone(), skip_missed_rays=True, tuning=tuning)
    alone = render(ws1.clone(), slice(1, 2), skip_missed_rays=True, tuning=tuning)
    if tuning == 8:
        bad = ~torch.isfinite(both['rgb'][0]).all(-1)
        print('scene 0: %d of %d pixels are not finite' % (int(bad.sum()), bad.numel()))
        assert float(bad.float().mean()) > 0.5, 'the poison should reach the decoder outputs of most of scene 0\'s rays'
    for k in ('rgb', 'depth', 'mask'):
        assert bool(torch.isfinite(both[k][1]).all()), k
        exact(both[k][1], alone[k][0], 'scene 1 next to the poisoned scene, ' + k)
    assert float(alone['mask'].max()) > 0.1, 'scene should not be empty'
