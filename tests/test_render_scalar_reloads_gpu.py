"""GPU checks of the S <= 64 render kernel whose arguments are read again from the argument segment at their use.

Since round 19 render_fwd_kernel re-reads the input pointers, S, `fine`, the fine-noise stride, the output pointers and the
divisor by rays per scene with scalar loads where it uses them (kernel_args_here), and computes its conditions on S, 2 S
and the number of attention rows at their use (scalar_here).  An argument read from the wrong offset, or a condition
computed from the wrong value, need not show at the benchmark's shape - so here are the shapes where each of them has
another value or takes another path:

  images of 16 x 16 and 32 x 32 (per-XCD queues of 16- and 32-pixel blocks) and 24 x 24 (8-pixel blocks; with tuning 16 the
  single queue), planes of side 32, S = 64 and S = 40 (a partial wave: the lanes without a sample), fine pass on and off,
  white and black background, noise given and null (null fine noise: row stride 0), one and two views per scene (the
  divisor by rays per scene), and cameras so that the first image misses the scene cube with every ray (the launch starts
  in a run of misses, its queues run dry and steal), one image hits it with every ray, and the last sees it small at the
  centre (a scene change inside a wave, a launch that ends in a run of misses).

Checks, per case:
  * every pixel is written: the outputs start as NaN;
  * rgb, depth and mask are torch.equal between tuning 0 (queues with the block table), 16 (single queue) and 32 (queues
    in block order);
  * with and without the miss runs skipped the rays that meet the cube are torch.equal;
  * everything is within the suite's 1e-4 of the CPU oracle."""
import pytest
import torch

from nerf_from_image_amd import ops
from oracle import nfi_oracle as orc
from parity_util import err
from stand_in import look_at_cameras
from test_hip_edge_cases import scene
from test_render_block_table_gpu import HIT_OFFSET, nan_empty

pytestmark = pytest.mark.gpu
A = 10
PLANE_RES = 32
RANGE = 0.55
TOL = 1e-4
SCENE_SEED = 5036         # fields that are not empty: every image that meets the cube has pixels with mask > 0.5 (asserted)


class Case:
    def __init__(self, name, B, side, S, fine=True, white=True, noise=True, views=1):
        self.name, self.B, self.side, self.S, self.fine, self.white, self.noise, self.views = name, B, side, S, fine, white, noise, views
        self.n = B * side * side

    def __repr__(self):
        return self.name


CASES = [Case('3x16x16_S64', 3, 16, 64),
         Case('3x32x32_S64', 3, 32, 64),
         Case('3x32x32_S40_black', 3, 32, 40, white=False),
         Case('3x16x16_S40_coarse_only', 3, 16, 40, fine=False),
         Case('3x16x16_S64_no_noise_black', 3, 16, 64, white=False, noise=False),
         Case('3x32x32_S40_no_noise', 3, 32, 40, noise=False),
         Case('1x24x24_S64', 1, 24, 64),
         Case('3x24x24_S40_black', 3, 24, 40, white=False),
         Case('4x16x16_S64_views2', 4, 16, 64, views=2),
         Case('6x32x32_S40_views2_black', 6, 32, 40, white=False, views=2)]


def cameras_of(case):
    """image 0 (of three or more): beside the cube, every ray misses; image 1: inside the cube's silhouette, every ray hits;
    the last: far away, the cube small at the centre; any others, and a single image: the cube with a margin"""
    g = torch.Generator().manual_seed(31 + case.n)
    cam = look_at_cameras(case.B, 1.0, g)
    radius, focal = torch.full((case.B,), 2.0), torch.full((case.B,), 1.0)
    if case.B >= 3:
        radius[1], focal[1] = 0.9, 4.0
        radius[-1] = 3.0
    cam[:, :3, 3] *= radius.view(-1, 1)
    if case.B >= 3:
        cam[0, :3, 3] += 6.0 * cam[0, :3, 0]          # six units along the camera's own x axis: it looks past the cube
        focal[0] = 4.0
    return cam, focal


_inputs = {}


def inputs_of(case, dev):
    """the case's field, cameras, noise and CPU oracle result: computed once, shared by its tests, never modified"""
    if case.name not in _inputs:
        n_scenes = case.B // case.views
        d, g = scene(n_scenes, A, PLANE_RES, SCENE_SEED)
        cam, focal = cameras_of(case)
        noise_c = torch.rand(case.B, case.side, case.side, case.S, generator=g) if case.noise else None
        noise_f = torch.rand(case.n, case.S, generator=g) if case.noise and case.fine else None
        rep = lambda t: t.repeat_interleave(case.views, dim=0)
        with torch.no_grad():
            o = orc.render(rep(d['planes']), d['w1'], d['b1'], d['w2'], d['b2'], cam, focal, case.side, case.side, case.S, RANGE,
                           white_background=case.white, fine_sampling=case.fine, noise_coarse=noise_c, noise_fine=noise_f,
                           use_sdf=True, beta=d['beta'], alpha=d['alpha'], attention_values=rep(d['att']))
        mv = lambda t: None if t is None else t.to(dev)
        _inputs[case.name] = dict(
            texels=ops.planes_to_texels(mv(d['planes'])), image=ops.decoder_pack(mv(d['w1']), mv(d['b1']), mv(d['w2']), mv(d['b2']), A),
            att=mv(d['att']), beta=mv(d['beta']), alpha=mv(d['alpha']), cam=mv(cam), focal=mv(focal), noise_c=mv(noise_c),
            noise_f=mv(noise_f), oracle={k: o[k] for k in ('rgb', 'depth', 'mask')})
    return _inputs[case.name]


def render(case, dev, tuning, skip, monkeypatch):
    i = inputs_of(case, dev)
    with monkeypatch.context() as m:
        m.setattr(torch, 'empty', nan_empty(torch.empty))
        out = ops.render_fwd(i['cam'], i['focal'], case.side, case.side, case.S, i['texels'], i['image'], RANGE, A, i['att'], True,
                             i['beta'], i['alpha'], noise_coarse=i['noise_c'], noise_fine=i['noise_f'], fine_sampling=case.fine,
                             white_background=case.white, skip_missed_rays=skip, tuning=tuning, views_per_scene=case.views)
    torch.cuda.synchronize(dev)
    return out


def wide_hits(case, dev):
    """bool [B, side, side]: the rays the kernel marches when it skips the others (hit bit 1 of the ray set-up)"""
    i = inputs_of(case, dev)
    ws = ops.render_setup(i['cam'], i['focal'], case.side, case.side, RANGE)
    hit = ws[HIT_OFFSET(case.n):HIT_OFFSET(case.n) + case.n]
    return ((hit & 2) != 0).view(case.B, case.side, case.side)


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_hand_outs_agree_and_match_the_oracle(gpu_device, case, monkeypatch):
    dev = gpu_device
    i = inputs_of(case, dev)
    hits = wide_hits(case, dev)
    if case.B >= 3:        # the cameras do what cameras_of says
        per_image = hits.view(case.B, -1).sum(dim=1).tolist()
        print(case, 'marched rays per image', per_image)
        assert per_image[0] == 0 and per_image[1] == case.side * case.side and 0 < per_image[-1] < case.side * case.side
        assert not bool(hits[-1, 0].any()) and not bool(hits[-1, -1].any())       # the last image's first and last row miss
    ref = render(case, dev, 16, True, monkeypatch)              # the single counter
    for k in ('rgb', 'depth', 'mask'):
        assert not bool(torch.isnan(ref[k]).any()), (case, k)
        e = err(ref[k], i['oracle'][k])
        print(case, k, e)
        assert e['max'] <= TOL and e['nonfinite'] == 0, (case, k, e)
    lit = ref['mask'].view(case.B, -1).amax(dim=1)
    assert bool((lit[1 if case.B >= 3 else 0:] > 0.5).all()), (case, lit.tolist())     # the images that meet the cube are not empty
    for tuning in (0, 32):
        out = render(case, dev, tuning, True, monkeypatch)
        for k in ('rgb', 'depth', 'mask'):
            assert torch.equal(out[k], ref[k]), (case, tuning, k)       # (NaN != NaN: an unwritten pixel fails here too)


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_skipping_the_miss_runs_changes_no_ray_that_hits(gpu_device, case, monkeypatch):
    dev = gpu_device
    i = inputs_of(case, dev)
    hits = wide_hits(case, dev)
    skip, march = render(case, dev, 0, True, monkeypatch), render(case, dev, 0, False, monkeypatch)
    for k in ('rgb', 'depth', 'mask'):
        assert not bool(torch.isnan(march[k]).any()), (case, k)
        assert torch.equal(skip[k][hits], march[k][hits]), (case, k)
        e = err(march[k], i['oracle'][k])
        assert e['max'] <= TOL and e['nonfinite'] == 0, (case, k, e)
