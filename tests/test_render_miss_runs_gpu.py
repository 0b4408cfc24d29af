"""GPU checks of the render kernels' path for runs of rays that miss the scene cube (skip_miss_run in nfi_kernels.hip).

A test chooses the miss pattern itself: the ray set-up runs alone (ops.render_setup), bit 1 of chosen hit bytes of the
workspace is cleared - they sit at byte 576 + 32 n of the documented prefix - and the render kernel is launched on that
workspace (ops.render_fwd(..., rays_ready=True)).  Rays are independent and the reduction cells stay untouched, so the
expected image is exact in both halves: a pixel whose bit was cleared holds the background (rgb 1 on white, depth 0,
mask 0, zero attribute maps) and every other pixel equals the unmodified render's bit for bit.

The cameras look at the cube from close by with a long lens, so that the set-up itself marks every ray as a hit (asserted)
and "no ray skipped" / "all but the first" are what they say.

The training stash cannot be reached this way: nfi_render_fwd refuses rays_ready together with a stash, whose ray set-up
writes to the caller's tensors.  Its test takes the miss pattern a wide camera gives (from the 'hit' tap of the same call):
skipped rays hold all-zero stash rows and background pixels, and the rows of every other ray equal, bit for bit, the
per-sample taps of a launch that skips nothing (the stage taps switch the skipping off)."""
import pytest
import torch

from nerf_from_image_amd import ops
from stand_in import look_at_cameras
from test_hip_edge_cases import scene

pytestmark = pytest.mark.gpu
A = 10
HIT_OFFSET = lambda n: 576 + 32 * n
# (H, W, S) -> seed of the random scene: ones whose field is not next to empty from these cameras (the oracle's mask has a
# mean of 0.16 to 0.99; with 31 H + W + S for all, 32 x 32 gave 0.007 and 12 x 20 gave 8e-6)
SCENE_SEED = {(32, 32, 8): 1035, (16, 16, 8): 520, (8, 8, 8): 264, (12, 20, 8): 401, (16, 16, 65): 577, (16, 16, 129): 641}


def patterns(B, H, W):
    """name -> bool [n] in pixel order, True = this ray's hit bit is cleared"""
    n = B * H * W
    z = lambda: torch.zeros(n, dtype=torch.bool)
    p = {'none': z(), 'all': ~z()}
    p['all_but_first'] = ~z(); p['all_but_first'][0] = False
    p['all_but_last'] = ~z(); p['all_but_last'][n - 1] = False
    p['isolated'] = z(); p['isolated'][[3, n // 3, n // 3 + 2, n - 2]] = True
    for length in (1, 2, 3, 5, 63, 64, 65):
        for start in (10, 11):
            m = z(); m[start:start + length] = True
            p['run%d_at%d' % (length, start)] = m
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    p['checkerboard'] = (((x + y) & 1) == 1).repeat(B, 1, 1).reshape(n)
    for i, density in enumerate((0.01, 0.5, 0.99)):
        g = torch.Generator().manual_seed(100 + i)
        m = torch.rand(n, generator=g) < density
        m[n // 2] = True; m[n // 2 + 1] = False          # one of each whatever the draw
        p['random%g' % density] = m
    return p


PATTERN_NAMES = list(patterns(2, 8, 8))
_cache = {}


def case(dev, B, H, W, S, fine=True, **kw):
    """inputs, the workspace after the set-up and the unmodified render of one shape / variant: made once, never written"""
    key = (B, H, W, S, fine, tuple(sorted(kw.items())))
    if key not in _cache:
        d, g = scene(B, A, 32, SCENE_SEED[H, W, S])
        cam = look_at_cameras(B, 1.6, g).to(dev)
        focal = torch.full((B,), 4.0, device=dev)
        mv = lambda t: t.to(dev)
        texels = ops.planes_to_texels(mv(d['planes']))
        image = ops.decoder_pack(mv(d['w1']), mv(d['b1']), mv(d['w2']), mv(d['b2']), A)
        noise_c = torch.rand(B, H, W, S, generator=g).to(dev)
        noise_f = torch.rand(B * H * W, S, generator=g).to(dev) if fine else None

        def render(ws):
            return ops.render_fwd(cam, focal, H, W, S, texels, image, 0.55, A, mv(d['att']), True, mv(d['beta']), mv(d['alpha']),
                                  noise_coarse=noise_c, noise_fine=noise_f, fine_sampling=fine, white_background=True,
                                  skip_missed_rays=True, workspace=ws, rays_ready=True, **kw)
        ws = ops.render_setup(cam, focal, H, W, 0.55)
        n = B * H * W
        hit = ws[HIT_OFFSET(n):HIT_OFFSET(n) + n].cpu()
        assert bool(((hit & 2) != 0).all()), 'the cameras of this test leave no ray outside the cube'
        ref = render(ws.clone())
        assert float(ref['mask'].max()) > 0.1, 'scene should not be empty'
        _cache[key] = (render, ws, ref)
    return _cache[key]


def check(dev, B, H, W, S, name, maps=(), fine=True, **kw):
    render, ws, ref = case(dev, B, H, W, S, fine, **kw)
    n = B * H * W
    cleared = patterns(B, H, W)[name]
    # on the CPU, from the mask: the pattern leaves rays on both sides of the branch where it can
    if name != 'none':
        assert int(cleared.sum()) >= 1, name
    if name != 'all':
        assert int((~cleared).sum()) >= 1, name
    ws2 = ws.clone()
    hit = ws2[HIT_OFFSET(n):HIT_OFFSET(n) + n]
    hit[cleared.to(dev)] &= 0xfd
    out = render(ws2)
    c = cleared.view(B, H, W).to(dev)
    for k, bgv in (('rgb', 1.0), ('depth', 0.0), ('mask', 0.0)) + tuple((m, 0.0) for m in maps):
        got, want = out[k], ref[k]
        assert bool((got[c] == bgv).all()), (name, k, 'skipped rays hold the background')
        assert torch.equal(got[~c], want[~c]), (name, k, 'every other ray is the unmodified render\'s')


@pytest.mark.parametrize('name', PATTERN_NAMES)
def test_miss_patterns_per_xcd_queues(gpu_device, name):
    """a) 2 images of 32 x 32, 8 + 8 samples: the per-XCD queues with one block per image, stealing from the start"""
    check(gpu_device, 2, 32, 32, 8, name)


@pytest.mark.parametrize('name', PATTERN_NAMES)
@pytest.mark.parametrize('H,W', [(16, 16), (8, 8), (12, 20)])
def test_miss_patterns_block_sides_and_single_queue(gpu_device, H, W, name):
    """b) block sides 16 and 8, and 12 x 20: sides that are no multiples of 8, the single queue"""
    check(gpu_device, 2, H, W, 8, name)


def test_miss_runs_extra_maps(gpu_device):
    """c) the kernels with the composited `coords` and `semantics` maps: zero maps for a skipped ray"""
    check(gpu_device, 2, 32, 32, 8, 'random0.5', maps=('coords', 'semantics'), want_coords=True, want_semantics=True)
    check(gpu_device, 2, 32, 32, 8, 'run65_at11', maps=('coords', 'semantics'), want_coords=True, want_semantics=True)


def test_miss_runs_wide_kernel(gpu_device):
    """c) the 64 < S <= 128 kernel at 65 + 65 samples"""
    check(gpu_device, 2, 16, 16, 65, 'random0.5')
    check(gpu_device, 2, 16, 16, 65, 'run65_at11')


def test_miss_runs_long_kernel(gpu_device):
    """c) the single-pass kernel at one pass of 129 samples"""
    check(gpu_device, 2, 16, 16, 129, 'random0.5', fine=False)
    check(gpu_device, 2, 16, 16, 129, 'run65_at11', fine=False)


@pytest.mark.parametrize('S', [8, 65])
def test_miss_runs_training_stash(gpu_device, S):
    """c) the training stash (S <= 64 kernel and wide kernel), on the misses a wide camera leaves: see the module docstring"""
    dev = gpu_device
    B, H, W = 2, 32, 32
    d, g = scene(B, A, 32, 77 + S)
    cam = look_at_cameras(B, 1.8, g).to(dev)
    focal = torch.full((B,), 1.0, device=dev)
    mv = lambda t: t.to(dev)
    texels = ops.planes_to_texels(mv(d['planes']))
    image = ops.decoder_pack(mv(d['w1']), mv(d['b1']), mv(d['w2']), mv(d['b2']), A)
    noise_c = torch.rand(B, H, W, S, generator=g).to(dev)
    noise_f = torch.rand(B * H * W, S, generator=g).to(dev)
    args = (cam, focal, H, W, S, texels, image, 0.55, A, mv(d['att']), True, mv(d['beta']), mv(d['alpha']))
    kw = dict(noise_coarse=noise_c, noise_fine=noise_f, fine_sampling=True, white_background=True, skip_missed_rays=True)
    st = ops.render_fwd(*args, stash=True, taps=('hit',), **kw)
    full = ops.render_fwd(*args, taps=('t_coarse', 'sigma_coarse', 'rgb_coarse', 't_fine', 'sigma_fine', 'rgb_fine'), **kw)
    skipped = (st['hit'] & 2) == 0
    frac = skipped.float().mean().item()
    print('S = %d: %.3f of the rays are skipped' % (S, frac))
    assert 0.0 < frac < 1.0
    for k, bgv in (('rgb', 1.0), ('depth', 0.0), ('mask', 0.0), ('stash_t', 0.0), ('stash_sigma', 0.0), ('stash_rgb', 0.0)):
        assert bool((st[k][skipped] == bgv).all()), (k, 'skipped rays: background pixel, all-zero stash row')
    for k in ('rgb', 'depth', 'mask'):
        assert torch.equal(st[k][~skipped], full[k][~skipped]), k
    for k, (a, b) in dict(stash_t=('t_coarse', 't_fine'), stash_sigma=('sigma_coarse', 'sigma_fine'),
                          stash_rgb=('rgb_coarse', 'rgb_fine')).items():
        assert torch.equal(st[k][:, :, :, :S][~skipped], full[a][~skipped]), k
        assert torch.equal(st[k][:, :, :, S:][~skipped], full[b][~skipped]), k
