"""Several views per scene from one set of planes (nfi_render_args.views_per_scene, ops.render_fwd(views_per_scene=),
the render option, render.render_views, generator.bake), forward and backward.

The definition of correct: V views per scene give, bit for bit, what one view per scene gives for the texels and the
attention values repeat_interleave(V, 0).  2 scenes x 3 views, so the scene changes at image 3 (not at a power of two);
every view has rays that hit the scene cube and rays that miss it (asserted through the `hit` tap; checked beforehand on
the CPU with the oracle's ray functions: 33-40 of 63 and 68-78 of 128 rays hit)."""
import types

import pytest
import torch

import nerf_from_image_amd.generator as nfi_gen
import nerf_from_image_amd.render as nfi_render
from nerf_from_image_amd import ops
from oracle import nfi_oracle as orc
from stand_in import StandInGenerator, _Decoder, _Lin, look_at_cameras
from test_hip_backward import rel_close

pytestmark = pytest.mark.gpu

R, SCENES, V, IMAGES, RANGE, FOCAL = 32, 2, 3, 6, 0.55, 1.0254
_inputs = {}


def inputs(dev, A, vd=False):
    """Planes that differ per scene, a decoder, the six cameras - built once per (A, vd) and left unchanged."""
    key = (A, vd)
    if key not in _inputs:
        g = torch.Generator().manual_seed(31)
        cam = look_at_cameras(IMAGES, 2.0, g).to(dev)
        g2 = torch.Generator().manual_seed(310 + A + 1000 * vd)
        # channels-last [2,96,R,R]: the same numbers serve the planar and the interleaved texel layout
        planes = torch.randn(SCENES, 96, R, R, generator=g2).to(dev).contiguous(memory_format=torch.channels_last)
        planes = planes.view(SCENES, 3, 32, R, R)
        dec = _Decoder(33 if vd else (1 + A if A > 0 else 4), g2)
        with torch.no_grad():
            # centre the distance output (row 0 of the second layer) on the lower quartile of the SDF over the cube: a quarter
            # of the volume is inside a surface, the images are not empty (mask mean 0.23 with the oracle on the CPU)
            x = (torch.rand(SCENES, 4000, 3, generator=g2) * 2 - 1) * RANGE
            sdf = orc.field_query(planes.cpu(), dec.net[0].weight, dec.net[0].bias, dec.net[2].weight[:4], dec.net[2].bias[:4], x,
                                  RANGE, True, torch.tensor([0.12]), torch.tensor([0.3]))['sdf']
            dec.net[2].bias[0] -= sdf.flatten().quantile(0.25)
        dec = dec.to(dev)
        d = dict(cam=cam, focal=torch.full((IMAGES,), FOCAL, device=dev), planes=planes,
                 w=[t.detach() for t in (dec.net[0].weight, dec.net[0].bias, dec.net[2].weight, dec.net[2].bias)],
                 att=(torch.rand(SCENES, max(A, 1), 3, generator=g2) * 2 - 1).to(dev) if A > 0 else None,
                 beta=torch.tensor([0.12], device=dev), alpha=torch.tensor([0.3], device=dev))
        if vd:
            out = _Lin(32, A if A > 0 else 3, g2).to(dev)
            d['w'] += [out.weight.detach(), out.bias.detach()]
        _inputs[key] = d
    return _inputs[key]


def field(d, A, tex, layout, vd):
    if layout == 'interleaved':
        texels = ops.planes_view_as_texels(d['planes'])
        assert texels is not None and ops.texel_layout_of(texels) == ops.TEXELS_INTERLEAVED
    else:
        texels = ops.planes_to_texels(d['planes'].contiguous(), tex)
    image = ops.decoder_pack_viewdir(*d['w'], A, tex) if vd else ops.decoder_pack(*d['w'], A, tex)
    return texels, image


# (S, fine, texels, A, mode, skip_missed_rays, texel layout, view-direction decoder, row window, (H, W))
#   (9, 7): single work counter, scanline order, ragged last workgroup;  (16, 8): per-XCD queues, tile order
F32, F16, BF16 = ops.TEXEL_F32, ops.TEXEL_F16, ops.TEXEL_BF16
CASES = [
    (24, True, F32, 10, 'plain', True, 'planar', False, None, (9, 7)),
    (24, True, F32, 10, 'plain', True, 'planar', False, None, (16, 8)),
    (24, True, F16, 10, 'plain', True, 'planar', False, None, (16, 8)),
    (24, True, BF16, 10, 'plain', True, 'planar', False, None, (9, 7)),
    (24, True, F32, 0, 'plain', True, 'planar', False, None, (9, 7)),
    (24, True, F32, 10, 'plain', False, 'planar', False, None, (16, 8)),
    (24, True, F32, 10, 'stash', True, 'planar', False, None, (9, 7)),
    (24, True, F32, 0, 'stash', True, 'planar', False, None, (16, 8)),
    (24, True, F32, 10, 'semantics+coords', True, 'planar', False, None, (16, 8)),
    (24, True, F32, 10, 'normals', True, 'planar', False, None, (9, 7)),
    (24, True, F32, 10, 'termination', True, 'planar', False, None, (16, 8)),
    (24, True, F32, 10, 'taps', True, 'planar', False, None, (9, 7)),
    (100, True, F32, 10, 'plain', True, 'planar', False, None, (16, 8)),
    (100, True, F16, 0, 'plain', False, 'planar', False, None, (9, 7)),
    (100, True, F32, 10, 'stash', True, 'planar', False, None, (16, 8)),
    (100, True, F32, 10, 'semantics+coords', True, 'planar', False, None, (9, 7)),
    (100, True, F32, 10, 'normals', True, 'planar', False, None, (16, 8)),
    (100, True, F32, 10, 'termination', True, 'planar', False, None, (9, 7)),
    (100, True, F32, 10, 'taps', True, 'planar', False, None, (16, 8)),
    (200, False, F32, 10, 'plain', True, 'planar', False, None, (16, 8)),
    (200, False, F16, 10, 'plain', False, 'planar', False, None, (9, 7)),
    (200, False, F32, 0, 'stash', True, 'planar', False, None, (16, 8)),
    (24, True, F32, 10, 'plain', True, 'interleaved', False, None, (16, 8)),
    (24, True, F32, 10, 'plain', True, 'planar', True, None, (9, 7)),
    (24, True, F32, 10, 'plain', True, 'planar', False, (4, 16), (8, 8)),
]
MODES = {'plain': {}, 'stash': dict(stash=True), 'semantics+coords': dict(want_semantics=True, want_coords=True),
         'normals': dict(want_normals=True), 'termination': dict(termination_eps=1e-3), 'taps': dict(taps=ops.TAP_NAMES)}


def _id(c):
    S, fine, tex, A, mode, skip, layout, vd, window, (H, W) = c
    return '%s%d-%s-A%d-%s-%s%s%s%s-%dx%d' % ('2x' if fine else '', S, {F32: 'f32', F16: 'f16', BF16: 'bf16'}[tex], A, mode,
                                             'skip' if skip else 'march', '-interleaved' if layout != 'planar' else '',
                                             '-viewdir' if vd else '', '-window' if window else '', H, W)


def render_pair(dev, case, flip=False):
    """(multi-view call on the 2 scenes, one-view call on the 6 repeated scenes, inputs): same cameras, same noise."""
    S, fine, tex, A, mode, skip, layout, vd, window, (H, W) = case
    d = inputs(dev, A, vd)
    texels, image = field(d, A, tex, layout, vd)
    g = torch.Generator().manual_seed(S + H)
    common = dict(noise_coarse=torch.rand(IMAGES, H, W, S, generator=g).to(dev),
                  noise_fine=torch.rand(IMAGES * H * W, S, generator=g).to(dev) if fine else None, fine_sampling=fine,
                  white_background=True, skip_missed_rays=skip, row_window=window,
                  ray_features=ops.pad_ray_features(torch.randn(IMAGES, H, W, 32, generator=g).to(dev)) if vd else None,
                  **MODES[mode])

    def call(tx, att, **kw):
        return ops.render_fwd(d['cam'], d['focal'], H, W, S, tx, image, RANGE, A, att, True, d['beta'], d['alpha'], **common, **kw)
    multi = call(texels, d['att'], views_per_scene=V)
    if flip:
        texels = texels.flip(0)
    base = call(texels.repeat_interleave(V, 0), None if d['att'] is None else d['att'].repeat_interleave(V, 0),
                views_per_scene=1)
    return multi, base, (call, texels, d)


_hits = {}


def hits_per_view(dev, H, W, window):
    """Rays of every view that meet the scene cube, from the `hit` tap of one small render per shape (kept)."""
    key = (H, W, window)
    if key not in _hits:
        d = inputs(dev, 10)
        texels, image = field(d, 10, F32, 'planar', False)
        out = ops.render_fwd(d['cam'], d['focal'], H, W, 8, texels, image, RANGE, 10, d['att'], True, d['beta'], d['alpha'],
                             fine_sampling=False, row_window=window, taps=('hit',), views_per_scene=V)
        _hits[key] = (out['hit'] & 1).view(IMAGES, -1).sum(dim=1).tolist()
    return _hits[key]


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_views_per_scene_equals_repeated_scenes_bit_for_bit(gpu_device, case):
    H, W = case[-1]
    hits = hits_per_view(gpu_device, H, W, case[-2])
    assert all(0 < h < H * W for h in hits), hits              # every view has rays that hit and rays that miss
    multi, base, _ = render_pair(gpu_device, case)
    keys = sorted(k for k in multi if k != '_workspace')
    assert keys == sorted(k for k in base if k != '_workspace') and {'rgb', 'depth', 'mask'} <= set(keys)
    if case[4] == 'stash':
        assert {'stash_t', 'stash_sigma', 'stash_rgb'} <= set(keys)
    if 'hit' in multi:
        hits = (multi['hit'] & 1).view(IMAGES, -1).sum(dim=1)
        assert bool(((hits > 0) & (hits < H * W)).all()), hits.tolist()
    assert float(multi['mask'].mean()) > 0.02, 'the scenes should not be empty'
    for k in keys:
        assert torch.equal(multi[k], base[k]), k


def test_a_scene_index_that_ignores_the_views_would_show(gpu_device):
    """Negative control: against the repeated scenes in the OTHER order the images differ - a scene index that ignored V
    (image i -> scene i, out of range here) or counted modulo V could not pass the test above unnoticed."""
    multi, flipped, _ = render_pair(gpu_device, CASES[1], flip=True)
    assert not torch.equal(multi['rgb'], flipped['rgb'])
    per_image = (multi['rgb'] != flipped['rgb']).flatten(1).any(dim=1)
    assert bool(per_image.all()), per_image.tolist()


def test_one_view_passed_explicitly_is_the_call_without_it(gpu_device):
    _, base, (call, texels, d) = render_pair(gpu_device, CASES[1])
    plain = call(texels.repeat_interleave(V, 0), d['att'].repeat_interleave(V, 0))
    for k in ('rgb', 'depth', 'mask'):
        assert torch.equal(plain[k], base[k]), k


# ------------------------------------------------------------------------------------------------
# refusals: all before any launch
# ------------------------------------------------------------------------------------------------
class NoLaunch:
    """Fails the test if a refused call reaches the library."""

    def __enter__(self):
        from nerf_from_image_amd import _lib
        self.lib, self.saved = _lib, _lib.call_struct

        def forbidden(fname, *a, **k):
            if fname in ('nfi_render_fwd', 'nfi_render_setup'):
                raise AssertionError('%s was called for a call that must be refused first' % fname)
            return self.saved(fname, *a, **k)
        _lib.call_struct = forbidden
        return self

    def __exit__(self, *a):
        self.lib.call_struct = self.saved


def test_render_fwd_refuses_scene_counts_that_do_not_cover_the_cameras(gpu_device):
    d = inputs(gpu_device, 10)
    S, H, W = 24, 9, 7
    texels, image = field(d, 10, F32, 'planar', False)

    def fwd(cams, tx, att, views, strict=False):
        return ops.render_fwd(d['cam'][:cams], d['focal'][:cams], H, W, S, tx, image, RANGE, 10, att, True, d['beta'], d['alpha'],
                              noise_fine=torch.rand(cams * H * W, S, device=gpu_device), views_per_scene=views, strict=strict)
    with NoLaunch():
        with pytest.raises(ValueError, match='texels'):
            fwd(2, texels[:1], d['att'], 1)                      # the missing bounds check: one scene, two cameras
        with pytest.raises(ValueError, match='texels'):
            fwd(2, texels[:1], d['att'], 1, strict=True)         # ... before the strict path's own set-up launch too
        with pytest.raises(ValueError, match='attention_values'):
            fwd(2, texels, d['att'][:1], 1)
        with pytest.raises(ValueError, match='views_per_scene'):
            fwd(5, texels, d['att'], 2)                          # 5 cameras are not a whole number of 2-view scenes
        with pytest.raises(ValueError, match='texels'):
            fwd(6, texels[:1], d['att'], 3)


def stand_in(dev, use_viewdir=False, seed=7):
    torch.manual_seed(seed)
    model = StandInGenerator(RANGE, attention_values=10, use_sdf=True, plane_res=R, use_viewdir=use_viewdir).to(dev)
    with torch.no_grad():
        model.alpha.fill_(0.2)
    return nfi_gen.attach(model)


def bound_render(views, use_viewdir=False, fine=True):
    cfg = types.SimpleNamespace(use_viewdir=use_viewdir, use_sdf=True, attention_values=10, fine_sampling=fine)
    return nfi_render.make_render(cfg, {'scene_range': RANGE, 'white_background': True}, views_per_scene=views)


def test_render_refuses_a_camera_count_that_is_not_views_times_scenes(gpu_device):
    model = stand_in(gpu_device).eval()
    d = inputs(gpu_device, 10)
    g = torch.Generator().manual_seed(3)
    z3, z2 = torch.randn(3, 512, generator=g).to(gpu_device), torch.randn(2, 512, generator=g).to(gpu_device)
    with NoLaunch(), torch.no_grad():
        with pytest.raises(ValueError, match='views_per_scene'):
            bound_render(3)(model, 9, 7, d['cam'], d['focal'], None, None, z3, 24)            # 6 cameras, 3 x 3 expected
        with pytest.raises(ValueError, match='views_per_scene'):
            bound_render(3)(model, 9, 7, d['cam'][:5], d['focal'][:5], None, None, z2, 24)    # 5 cameras


def test_render_refuses_more_stash_points_per_scene_than_the_backward_addresses(gpu_device):
    """128 x 128 rays x (128 + 128) samples x 9 views = 37.7 M points per scene > 2^25: refused in the forward call, behind
    the model call and before the render launch (the stash is never allocated)."""
    model = stand_in(gpu_device)
    g = torch.Generator().manual_seed(4)
    cam = look_at_cameras(9, 2.0, g).to(gpu_device)
    z = torch.randn(1, 512, generator=g).to(gpu_device)
    with NoLaunch(), pytest.raises(ValueError, match=r'2\^25'):
        bound_render(9)(model, 128, 128, cam, torch.full((9,), FOCAL, device=gpu_device), None, None, z, 128)


# ------------------------------------------------------------------------------------------------
# backward: render_views on a hand-built field
# ------------------------------------------------------------------------------------------------
BOUNDS = dict(planes=2e-5, w1=2e-5, b1=2e-5, w2=2e-5, b2=2e-5, attention_values=2e-5, cam2world=2e-5, focal=2e-5,
              beta=1e-3, alpha=1e-3)


def check_gradients(names, got, ref, what):
    """The bounds of test_ray_order_hint_changes_nothing / test_binned_scatter_matches_atomic_scatter (same addends per point,
    another order or grouping of the sums): max error over max |reference|."""
    for n, a, b in zip(names, got, ref):
        bound = BOUNDS.get(n, 2e-5)
        scale = float(b.abs().max().clamp_min(1e-12))
        print('%s: grad %-28s rel %.3e (bound %.0e, scale %.3e)' % (what, n, float((a - b).abs().max()) / scale, bound, scale))
    for n, a, b in zip(names, got, ref):
        assert float(b.abs().max()) > 0, n
        rel_close(a, b, '%s: grad %s' % (what, n), BOUNDS.get(n, 2e-5))


@pytest.mark.parametrize('H,W,S', [(16, 8, 32),        # 8 192 points per image, 24 576 per scene: both sides scatter atomically
                                   (16, 16, 64)])      # 32 768 per image: atomic; 98 304 per scene: the binned scatter
def test_render_views_backward_sums_the_views(gpu_device, H, W, S):
    from nerf_from_image_amd.field_backward import BINNED_SCATTER_MIN_POINTS as binned
    assert (H * W * 2 * S >= binned, V * H * W * 2 * S >= binned) == (False, (H, W, S) == (16, 16, 64))
    dev = gpu_device
    d = inputs(dev, 10)
    g = torch.Generator().manual_seed(H * W)
    w_rgb, w_mask = torch.randn(IMAGES, H, W, 3, generator=g).to(dev), torch.randn(IMAGES, H, W, generator=g).to(dev)
    names = ['planes', 'w1', 'b1', 'w2', 'b2', 'attention_values', 'beta', 'alpha', 'cam2world', 'focal']

    def run(repeat):
        planes = d['planes'].contiguous().clone().requires_grad_()
        w = [t.clone().requires_grad_() for t in d['w']]
        att, beta, alpha = (t.clone().requires_grad_() for t in (d['att'], d['beta'], d['alpha']))
        cam, focal = d['cam'].clone().requires_grad_(), d['focal'].clone().requires_grad_()
        # the baseline's six scenes are differentiable functions of the same leaves: autograd sums the views' gradients
        pl, at = (planes.repeat_interleave(V, 0), att.repeat_interleave(V, 0)) if repeat else (planes, att)
        fused = nfi_gen.FusedField(ops.planes_to_texels(pl.detach()), ops.decoder_pack(*[t.detach() for t in w], 10), at, 10, True,
                                   beta, alpha, RANGE, planes=pl, decoder_params=tuple(w))
        torch.manual_seed(5)
        cams = cam if repeat else cam.view(SCENES, V, 4, 4)
        rgb, depth, mask, normals, extra = nfi_render.render_views(fused, H, W, cams, focal if repeat else focal.view(SCENES, V),
                                                                   S, strict_near_far=False)
        assert normals is None and extra is None and rgb.shape == (IMAGES, H, W, 3)
        loss = (rgb * w_rgb).sum() + (mask * w_mask).sum()
        return (rgb, depth, mask), torch.autograd.grad(loss, [planes] + w + [att, beta, alpha, cam, focal])
    out_m, got = run(False)
    out_b, ref = run(True)
    for a, b, k in zip(out_m, out_b, ('rgb', 'depth', 'mask')):
        assert torch.equal(a, b), k
    assert float(out_m[2].detach().mean()) > 0.02
    check_gradients(names, got, ref, 'render_views %dx%d S=%d' % (H, W, S))


# ------------------------------------------------------------------------------------------------
# through render(): the option against the same function with every latent repeated
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', ['fused + stash', 'fused + stash, view-direction decoder', 'staged'])
def test_render_with_the_option_equals_render_of_repeated_latents(gpu_device, path):
    dev = gpu_device
    vd = 'view-direction' in path
    model = stand_in(dev, use_viewdir=vd, seed=11).eval()
    d = inputs(dev, 10)
    H, W, S = 16, 8, 32
    g = torch.Generator().manual_seed(77)
    z = torch.randn(SCENES, 512, generator=g).to(dev)
    z_rep = z.repeat_interleave(V, 0)
    w_rgb, w_mask = torch.randn(IMAGES, H, W, 3, generator=g).to(dev), torch.randn(IMAGES, H, W, generator=g).to(dev)
    w_sem = torch.randn(IMAGES, H, W, 10, generator=g).to(dev)
    staged = path == 'staged'
    with torch.no_grad():
        planes, att = model.planes_and_values(z)
        planes_rep, att_rep = model.planes_and_values(z_rep)
    # the premise of the comparison: the stand-in is a fixed basis times the latents, and its output for a repeated latent is
    # the same row bit for bit (a producer that rounded a batch of 2 and a batch of 6 differently would make the baseline
    # render OTHER planes; nothing below would then be comparable at these bounds)
    assert torch.equal(planes_rep, planes.repeat_interleave(V, 0)) and torch.equal(att_rep, att.repeat_interleave(V, 0))
    params = [model.decoder.net[0].weight, model.decoder.net[0].bias, model.decoder.net[2].weight, model.decoder.net[2].bias,
              model.beta, model.alpha, model.synthesis_network.basis, model.texture_mapper.lin.weight]
    names = ['w1', 'b1', 'w2', 'b2', 'beta', 'alpha', 'plane producer', 'texture mapper']
    if vd:
        params += [model.viewdir_mapper.fc6.weight, model.viewdir_mapper.output.weight]
        names += ['viewdir fc6', 'viewdir output']

    def run(views, latents):
        cam, focal = d['cam'].clone().requires_grad_(), d['focal'].clone().requires_grad_()
        torch.manual_seed(9)
        out = bound_render(views, use_viewdir=vd)(model, H, W, cam, focal, None, None, latents, S, compute_semantics=staged)
        loss = (out[0] * w_rgb).sum() + (out[2] * w_mask).sum()
        if staged:
            assert out[4].requires_grad, 'a semantics map with a gradient takes the staged path'
            loss = loss + (out[4] * w_sem).sum()
        return out[:5], torch.autograd.grad(loss, params + [cam, focal])
    out_m, got = run(V, z)
    out_b, ref = run(1, z_rep)
    assert out_m[0].shape == (IMAGES, H, W, 3) and float(out_m[2].detach().mean()) > 0.02
    for a, b, k in zip(out_m, out_b, ('rgb', 'depth', 'mask', 'normals', 'extra')):
        assert (a is None and b is None) or torch.equal(a, b), k
    check_gradients(names + ['cam2world', 'focal'], got, ref, 'render(), ' + path)


# ------------------------------------------------------------------------------------------------
# bake + render_views
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('maps', [False, True])
def test_bake_and_render_views_equal_render(gpu_device, maps):
    dev = gpu_device
    model = stand_in(dev, seed=12).eval()
    d = inputs(dev, 10)
    H, W, S = 16, 8, 24
    z = torch.randn(SCENES, 512, generator=torch.Generator().manual_seed(5)).to(dev)
    kw = dict(compute_semantics=True, compute_normals=True) if maps else {}
    with torch.no_grad():
        torch.manual_seed(2)
        ref = bound_render(V)(model, H, W, d['cam'], d['focal'], None, None, z, S, **kw)
        baked = nfi_gen.bake(model, z)
        assert baked.texels.shape[0] == SCENES and not baked.requires_grad
        assert baked.beta.data_ptr() != model.beta.data_ptr()       # a snapshot, as the packed decoder image is
        torch.manual_seed(2)
        got = nfi_render.render_views(baked, H, W, d['cam'].view(SCENES, V, 4, 4), d['focal'].view(SCENES, V), S, **kw)
    # (outside no_grad as well: nothing of a baked field requires a gradient, the call stays on the fused inference path)
    torch.manual_seed(2)
    again = nfi_render.render_views(baked, H, W, d['cam'], d['focal'], S, **kw)
    assert len(got) == 5 and float(got[2].mean()) > 0.02
    for a, b, c, k in zip(got, ref[:5], again, ('rgb', 'depth', 'mask', 'normals', 'extra')):
        assert (a is None and b is None) or (torch.equal(a, b) and torch.equal(a, c) and not c.requires_grad), k
    assert (got[3] is not None) == maps and (got[4] is not None) == maps


def test_bake_and_render_views_refuse_what_they_cannot_do(gpu_device):
    dev = gpu_device
    d = inputs(dev, 10)
    z = torch.randn(SCENES, 512, generator=torch.Generator().manual_seed(5)).to(dev)
    with pytest.raises(ValueError, match='use_viewdir'):
        nfi_gen.bake(stand_in(dev, use_viewdir=True).eval(), z)
    model = stand_in(dev, seed=12).eval()
    baked = nfi_gen.bake(model, z)
    with NoLaunch():
        with pytest.raises(ValueError, match='cameras'):
            nfi_render.render_views(baked, 9, 7, d['cam'][:5], d['focal'][:5], 24)
        with pytest.raises(ValueError, match='leading dimension'):       # [3,2,4,4] is not 2 scenes x 3 views
            nfi_render.render_views(baked, 9, 7, d['cam'].view(V, SCENES, 4, 4), d['focal'].view(V, SCENES), 24)
        live = model(None, z, ['sampler'])['sampler'].fused          # the model's parameters require a gradient
        with pytest.raises(NotImplementedError, match=r'render\(\)'):
            nfi_render.render_views(live, 9, 7, d['cam'], d['focal'], 24, compute_semantics=True)
