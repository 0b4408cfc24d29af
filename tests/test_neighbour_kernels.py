"""The renderer's neighbours in the inversion loop at the sizes and inputs where their kernels can go wrong: the pose solve
(csrc/nfi_pnp.inc), the image metrics and the augmentation warp (csrc/nfi_neighbours.inc) and the plane producer's hand-off
(csrc/nfi_handoff.inc), each against its float64 reference (oracle/nfi_oracle_pnp.py, oracle/nfi_oracle_neighbours.py).

  pose     H != W (the screen grid is col / W - 0.5, row / H - 0.5, with row = i / W), pixel counts below one 256-thread
           stride and no multiple of it, 70 images (a second, ragged block of the 64-thread select kernel) with dummy poses
           among them, 64 focal proposals, an unsorted proposal list with a duplicate, a float mask that holds exactly the
           threshold.
  metrics  fewer than 256 elements per image and counts that are no multiple of 256, both layouts, either metric alone,
           masks of exactly 0.5, and the range check's own limits at the last element of the last image.
  warp     forward, atomic backward and ordered backward on non-square images, with 1, 8, 9 and 17 channels (the ordered
           gather kernel walks channels in passes of 8), seven transforms per call.
  hand-off forward and atomic backward at the corners of the tiling and at the largest in_channels.

Bounds: the ones tests/test_pose_estimation.py, tests/test_neighbours.py, tests/test_handoff_warp_ordered.py and
tests/test_handoff.py hold the same kernels to; none is new.  The case tables stand once, at module level; the CPU tests at
the top assert for those very inputs that the references are well conditioned (a unique minimum and a clear winner among
the focal proposals; no PSNR at the 60 dB clamp, no mask value at the threshold by accident; the float32 oracle within
half of each bound of the float64 oracle), so a failure on the GPU cannot be blamed on the input.  Every float64
reference is computed once per case and shared."""
import functools
import math

import numpy as np
import pytest
import torch
from scipy.optimize import least_squares
from scipy.spatial.transform import Rotation

from oracle import nfi_oracle_neighbours as orn
from oracle import nfi_oracle_pnp as orp


def seed_of(*parts):
    """A seed that does not depend on Python's string hashing."""
    s = 17
    for p in parts:
        for ch in str(p):
            s = (s * 131 + ord(ch)) % 2147483629
    return s


def rng(*parts):
    return torch.Generator().manual_seed(seed_of(*parts))


def maxdiff(a, b):
    return float((a.double() - b.double()).abs().max()) if a.numel() else 0.0


# ------------------------------------------------------------------------------------------------
# pose: cases
# ------------------------------------------------------------------------------------------------
FOCAL = 1.2
OCTAVES = (0.6, 1.2, 2.4)
FLIP = np.diag([1.0, -1.0, -1.0, 1.0])
DUMMY_W2C = FLIP @ np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -10.0], [0, 0, 0, 1]])
# tag: (B, H, W), noise levels, focal proposals
POSE_CASES = {
    'wide': ((3, 20, 36), (0.0, 0.02), OCTAVES),                 # H != W; 720 pixels: a ragged last stride
    'tall': ((2, 40, 9), (0.0, 0.02), OCTAVES),                  # H > W, W odd
    'strip': ((2, 9, 40), (0.02,), OCTAVES),                     # the transpose of `tall`
    'under': ((3, 15, 17), (0.0,), (1.2,)),                      # 255 pixels: fewer than one stride
    'over': ((3, 17, 17), (0.02,), (2.4, 0.6, 1.2, 1.2)),        # 289 pixels; an unsorted list with a duplicate
    'many': ((70, 12, 12), (0.0,), (1.2,)),                      # the select kernel's second block, 6 of its 64 threads live
    'sweep': ((1, 16, 16), (0.0,), tuple(np.geomspace(0.5, 3.0, 63)) + (1.2,)),      # the largest legal n_focal
    'mixed': ((4, 12, 20), (0.0,), OCTAVES),                     # solvable, empty, 3 pixels, a float mask holding 0.5
}
POSE_EXACT = [tag for tag, (_, noises, _) in POSE_CASES.items() if 0.0 in noises]
POSE_NOISY = [tag for tag, (_, noises, _) in POSE_CASES.items() if 0.02 in noises]
MANY_UNSOLVABLE = {3: 0, 64: 3, 69: 2}        # image of `many`: foreground pixels left to it


def ellipsoid_correspondences(bs, height, width, noise, focal=FOCAL, distance=2.5):
    """orp.synthetic_correspondences on a height x width pixel grid (seeded height * 100 + width): a camera looking at an
    ellipsoid whose surface points, in object coordinates, are what a perfect coordinate regressor would output per pixel.
    coords [B,H,W,3] float32, masks [B,H,W] bool, ground truth R [B,3,3], t [B,3] (P_cam = R P + t, z forward)."""
    gen = np.random.default_rng(height * 100 + width)
    grid = orp.screen_grid(height, width)
    coords = np.zeros((bs, height * width, 3), np.float32)
    masks = np.zeros((bs, height * width), bool)
    Rs, ts = [], []
    radii = np.array([0.9, 0.6, 0.75])
    for b in range(bs):
        R = Rotation.from_rotvec(gen.normal(size=3) * 1.2).as_matrix()
        tz = distance * (1.0 + gen.normal() * 0.08)
        t = np.array([gen.normal() * 0.07 * tz / focal, gen.normal() * 0.07 * tz / focal, tz])
        d_cam = np.concatenate([grid / focal, np.ones((len(grid), 1))], axis=1)
        o_obj, d_obj = -R.T @ t, d_cam @ R
        oo, dd = o_obj / radii, d_obj / radii
        a, bq, c = (dd * dd).sum(1), 2 * (dd @ oo), oo @ oo - 1
        disc = bq * bq - 4 * a * c
        hit = disc > 0
        s = (-bq - np.sqrt(np.where(hit, disc, 0))) / (2 * a)
        P = o_obj + d_obj * s[:, None]
        coords[b] = np.where(hit[:, None], P, 0) + (gen.normal(size=P.shape) * noise if noise else 0)
        masks[b] = hit
        Rs.append(R)
        ts.append(t)
    return coords.reshape(bs, height, width, 3), masks.reshape(bs, height, width), np.stack(Rs), np.stack(ts)


def keep_first_pixels(mask, n):
    """the first n foreground pixels of a [H,W] bool mask, row-major"""
    out = np.zeros(mask.size, bool)
    out[np.flatnonzero(mask)[:n]] = True
    return out.reshape(mask.shape)


@functools.lru_cache(maxsize=None)
def pose_case(tag, noise):
    """dict(coords float32 [B,H,W,3], masks (bool, or float32 for `mixed`) [B,H,W], foreground bool [B,H,W] = what counts
    above the 0.5 threshold, R, t, proposals, dummy = the images nothing can be solved for)"""
    (B, H, W), noises, proposals = POSE_CASES[tag]
    assert noise in noises
    coords, masks, Rs, ts = ellipsoid_correspondences(B, H, W, noise)
    dummy = ()
    if tag == 'many':
        for b, n in MANY_UNSOLVABLE.items():
            masks[b] = keep_first_pixels(masks[b], n)
        dummy = tuple(MANY_UNSOLVABLE)
    foreground = masks
    if tag == 'mixed':
        masks[1] = False
        masks[2] = keep_first_pixels(masks[2], 3)
        foreground = masks.copy()
        masks = masks.astype(np.float32)
        masks[3] = np.where(foreground[3], np.float32(0.75), np.float32(0.5))       # the background sits ON the threshold
        dummy = (1, 2)
    return dict(coords=coords, masks=masks, foreground=foreground, R=Rs, t=ts, proposals=np.asarray(proposals, np.float64),
                dummy=dummy)


@functools.lru_cache(maxsize=None)
def pose_reference(tag, noise):
    """orp.compute_pose_pnp on the case: (world2cam [B,4,4], focal [B], error [B]), float64"""
    c = pose_case(tag, noise)
    return orp.compute_pose_pnp(c['coords'], c['foreground'], c['proposals'])


def rot_angle_deg(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1))))


def refine_from(P, xy, f, R, t):
    """Levenberg-Marquardt on the reprojection error from the pose (R, t), with the oracle's residual and tolerances"""
    def res(p):
        pr, z = orp.project(Rotation.from_rotvec(p[:3]).as_matrix(), p[3:], f, P)
        r = pr - xy
        r[z <= 1e-9] = 1.0
        return r.ravel()
    sol = least_squares(res, np.concatenate([Rotation.from_matrix(R).as_rotvec(), t]), method='lm', xtol=1e-15, ftol=1e-15,
                        gtol=1e-15, max_nfev=400)
    return Rotation.from_rotvec(sol.x[:3]).as_matrix(), sol.x[3:]


# ------------------------------------------------------------------------------------------------
# image metrics: cases
# ------------------------------------------------------------------------------------------------
# (B, H, W): per-image noise amplitudes (uniform in [-a, a]: mse = a^2 / 3; 1e-3 is 64.8 dB - a non-identical image ABOVE the
# clamp); None: the image is its target.  3, 105, 255, 768 (exactly three strides) and 969 elements; masks of 1 .. 323
METRIC_CASES = {
    (1, 1, 1): (0.05,),
    (5, 5, 7): (1e-3, 7e-3, 0.04, 0.3, None),
    (2, 17, 5): (0.1, None),
    (3, 16, 16): (3e-3, None, 0.02),
    (2, 17, 19): (None, 0.2),
}
METRIC_SHAPES = list(METRIC_CASES)
PSNR_TOL = 2e-4        # dB
HALF = np.float32(0.5)
ABOVE_HALF = np.nextafter(np.float32(0.5), np.float32(1))
EDGE_SHAPE = (2, 17, 19)


@functools.lru_cache(maxsize=None)
def metric_case(B, H, W):
    """pred / target [B,3,H,W] in (-0.1, 1.1) with values on both sides of 0 and 1 (the clamp matters), masks [B,H,W] with no
    value within 1e-3 of the threshold; psnr64 (clamped at 60, and `raw`, unclamped) and iou: the references"""
    g = rng('metrics', B, H, W)
    target = torch.rand(B, 3, H, W, generator=g) * 1.1 - 0.05
    noise = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    pred = target.clone()
    for b, level in enumerate(METRIC_CASES[B, H, W]):
        if level is not None:
            pred[b] = (target[b] + noise[b] * level).clamp(-0.095, 1.095)
    mask_pred = torch.rand(B, H, W, generator=g) * 1.1 - 0.05
    mask_real = (mask_pred + 0.3 * torch.randn(B, H, W, generator=g)).clamp(-0.05, 1.05)
    mask_pred, mask_real = (torch.where((m - 0.5).abs() < 2e-3, m + 0.01, m) for m in (mask_pred, mask_real))
    p64, t64 = pred.double().clamp(0, 1), target.double().clamp(0, 1)
    raw = -10 * torch.log10((p64 - t64).square().mean(dim=[1, 2, 3]))
    return dict(pred=pred, target=target, mask_pred=mask_pred, mask_real=mask_real, psnr64=orn.psnr(pred.double(), target.double()),
                raw=raw, iou=orn.iou(mask_pred, mask_real), identical=[lv is None for lv in METRIC_CASES[B, H, W]])


# ------------------------------------------------------------------------------------------------
# warp: cases
# ------------------------------------------------------------------------------------------------
# name: (rot, scale, translation); one image per transform in every call (`identity` with scale 1: scale = NULL for a whole
# call is a call of its own)
TRANSFORMS = {'identity': (0.0, None, (0.0, 0.0)), 'zoom_out': (math.pi / 4, 0.5, (0.1, -0.05)), 'zoom_in': (1.0, 2.0, (0.0, 0.0)),
              'quarter_turn': (math.pi / 2, 1.0, (0.0, 0.0)),         # on a non-square image it exchanges the axes
              'half_turn_shift': (math.pi, 1.0, (0.3, -0.2)),
              'edge': (0.2, 1.3, (0.9, 0.8)),                         # most of the image leaves the frame
              'all_outside': (0.3, 1.0, (5.0, 5.0))}
NAMES = list(TRANSFORMS)
N_WARP = len(TRANSFORMS)
OUTSIDE = NAMES.index('all_outside')
WARP_ROT = torch.tensor([v[0] for v in TRANSFORMS.values()])
WARP_SCALE = torch.tensor([1.0 if v[1] is None else v[1] for v in TRANSFORMS.values()])
WARP_TRANS = torch.tensor([v[2] for v in TRANSFORMS.values()])
WARP_SIZES = [(1, 1), (1, 9), (7, 5), (33, 65), (24, 128)]
WARP_CHANNELS = (1, 8, 9, 17)     # of the gather kernel's passes of 8: a partial one, exactly one, one + one channel, two + one
WARP_GRAD_TOL = 1e-4              # of the gradient's largest entry


def warp_fwd_tol(H, W):
    """tests/test_neighbours.py: 2e-5 on images of up to 32 px a side, 6e-5 up to 128 px (the sampling coordinate's ulp grows
    with the image)"""
    assert max(H, W) <= 128
    return 2e-5 if max(H, W) <= 32 else 6e-5


@functools.lru_cache(maxsize=None)
def warp_case(H, W, C):
    """x [7,C,H,W] uniform in [-1, 1], the upstream gradient y normal with a block of zeros"""
    g = rng('warp', H, W, C)
    x, y = torch.rand(N_WARP, C, H, W, generator=g) * 2 - 1, torch.randn(N_WARP, C, H, W, generator=g)
    if H * W > 1:
        y[:, :, H // 4:H // 2 + 1, W // 3:] = 0
    return x, y


@functools.lru_cache(maxsize=None)
def warp_ref(H, W, C, white, dt, scaled=True):
    x, _ = warp_case(H, W, C)
    scale = WARP_SCALE if scaled else torch.ones(N_WARP)
    return orn.warp_images(x.to(dt), WARP_ROT.to(dt), scale.to(dt), WARP_TRANS.to(dt), white)


@functools.lru_cache(maxsize=None)
def warp_grad_ref(H, W, C):
    """float64 autograd of the oracle (the background does not enter the adjoint)"""
    x, y = warp_case(H, W, C)
    x64 = x.double().requires_grad_()
    out = orn.warp_images(x64, WARP_ROT.double(), WARP_SCALE.double(), WARP_TRANS.double(), False)
    return torch.autograd.grad((out * y.double()).sum(), x64)[0]


# ------------------------------------------------------------------------------------------------
# hand-off: cases
# ------------------------------------------------------------------------------------------------
# (B, Cin, R): one wave tile; second k pass and ragged blocks; the weight kernel's grid-stride loop; the largest in_channels
HANDOFF_SHAPES = [(1, 16, 8), (2, 144, 40), (2, 32, 96), (1, 256, 8)]
HANDOFF_FWD_TOL, HANDOFF_GRAD_TOL = 3e-6, 2e-5       # of the reference's largest entry (tests/test_handoff.py)
HANDOFF_GRADS = ('g_x', 'g_styles', 'g_weight', 'g_bias', 'g_previous_image')


@functools.lru_cache(maxsize=None)
def handoff_case(B, Cin, R):
    g = torch.Generator().manual_seed(B * 1000 + Cin + R)
    return dict(x=torch.randn(B, Cin, R, R, generator=g), s=torch.randn(B, Cin, generator=g) / Cin ** 0.5,
                w=torch.randn(96, Cin, generator=g), bias=torch.randn(96, generator=g),
                prev=torch.randn(B, 96, R // 2, R // 2, generator=g), up=torch.randn(B, 96, R, R, generator=g))


@functools.lru_cache(maxsize=None)
def handoff_ref(B, Cin, R, has_prev, dt):
    """(forward, dict of gradients) of orn.torgb_upsample_add in `dt`, the loss weighted by `up`"""
    t = handoff_case(B, Cin, R)
    leaves = [t[k].to(dt).requires_grad_() for k in ('x', 's', 'w', 'bias')] + ([t['prev'].to(dt).requires_grad_()] if has_prev else [])
    out = orn.torgb_upsample_add(leaves[0], leaves[1], leaves[2].view(96, Cin, 1, 1), leaves[3], leaves[4] if has_prev else None)
    grads = torch.autograd.grad((out * t['up'].to(dt)).sum(), leaves)
    return out.detach(), dict(zip(HANDOFF_GRADS, grads))


# ------------------------------------------------------------------------------------------------
# 1. the inputs are well conditioned for the references (CPU)
# ------------------------------------------------------------------------------------------------
def test_pose_cases_are_well_conditioned():
    """Every image a pose is expected for has at least 6 foreground pixels in general position (the common path: ONE
    refinement from the linear start), every other one fewer than 4.  On noisy data two minimisers agree only where the
    minimum is unique, and the focal choice is stable only where the best proposal wins clearly: the oracle's pose moves by
    at most 1e-6 when the refinement starts from the ground truth instead of the linear start, and the second-best
    proposal's error is at least 1.01 x the best (100 x the 1e-4 the errors are compared at)."""
    move, ratios = 0.0, []
    for tag, (shape, noises, proposals) in POSE_CASES.items():
        grid = orp.screen_grid(shape[1], shape[2])
        distinct = sorted(set(float(f) for f in proposals))
        assert len(proposals) <= 64 and FOCAL in distinct
        for noise in noises:
            c = pose_case(tag, noise)
            assert c['coords'].shape == shape + (3,) and c['masks'].shape == shape
            ref = pose_reference(tag, noise) if noise else None
            for b in range(shape[0]):
                idx = np.flatnonzero(c['foreground'][b])
                if b in c['dummy']:
                    assert len(idx) < 4, (tag, b)
                    continue
                P, xy = c['coords'][b].reshape(-1, 3)[idx].astype(np.float64), grid[idx]
                assert len(idx) >= 6 and not orp.dlt_is_degenerate(P, xy, FOCAL), (tag, noise, b, len(idx))      # (a)
                if not noise:
                    continue
                w2c, focal, err = ref
                assert focal[b] == FOCAL, (tag, b, focal)
                m = FLIP @ w2c[b]
                R1, t1 = refine_from(P, xy, FOCAL, c['R'][b], c['t'][b])
                move = max(move, np.abs(R1 - m[:3, :3]).max(), np.abs(t1 - m[:3, 3]).max())                     # (b)
                errs = sorted((orp.solve_one(P, xy, f)[2], f) for f in distinct)
                assert errs[0][1] == FOCAL and errs[0][0] == err[b], (tag, b, errs, err[b])
                ratios.append(errs[1][0] / errs[0][0])                                                           # (c)
    print('noisy pose cases: the minimum moves by %.2e with the start (bound 1e-6); second-best / best error %.4f .. %.4f '
          '(bound 1.01)' % (move, min(ratios), max(ratios)))
    assert move <= 1e-6 and min(ratios) >= 1.01
    c = pose_case('mixed', 0.0)
    assert c['masks'].dtype == np.float32 and bool((c['masks'][3] == 0.5).any()) and set(np.unique(c['masks'][3])) == {0.5, 0.75}
    assert [int(c['foreground'][b].sum()) for b in (1, 2)] == [0, 3]
    assert [int(pose_case('many', 0.0)['foreground'][b].sum()) for b in MANY_UNSOLVABLE] == list(MANY_UNSOLVABLE.values())
    sweep = np.asarray(POSE_CASES['sweep'][2], np.float32)
    assert len(sweep) == 64 == len(np.unique(sweep))           # no two proposals tie, as float32 either


def test_metric_cases_are_well_conditioned():
    """No image but the identical ones has a float64 PSNR within 1 dB of the 60 dB clamp (one lies above it, the others
    below), the identical ones are at the clamp; inputs stay inside the range check and reach both sides of 0 and of 1; no
    mask value lies within 1e-3 of the threshold, and both sides of it occur."""
    above = below = 0
    for shape in METRIC_SHAPES:
        c = metric_case(*shape)
        for b, same in enumerate(c['identical']):
            if same:
                assert torch.equal(c['pred'][b], c['target'][b]) and float(c['psnr64'][b]) == 60.0
            else:
                assert abs(float(c['raw'][b]) - 60.0) >= 1.0, (shape, b, float(c['raw'][b]))
                above, below = above + (float(c['raw'][b]) > 60), below + (float(c['raw'][b]) < 60)
        for k in ('pred', 'target', 'mask_pred', 'mask_real'):
            assert float(c[k].min()) > -0.1 and float(c[k].max()) < 1.1, (shape, k)
        for k in ('mask_pred', 'mask_real'):
            assert float((c[k] - 0.5).abs().min()) >= 1e-3, (shape, k)
        if shape[1] * shape[2] >= 35:
            assert all(bool((c[k] < 0).any()) and bool((c[k] > 1).any()) for k in ('pred', 'target')), shape
            assert all(bool((c[k] > 0.5).any()) and bool((c[k] < 0.5).any()) for k in ('mask_pred', 'mask_real')), shape
    assert above >= 1 and below >= 6
    assert float(ABOVE_HALF) > 0.5 and float(np.nextafter(np.float32(1.1), np.float32(0))) < 1.1 < float(np.float32(1.1))


def test_warp_cases_are_well_conditioned():
    """The float32 CPU oracle stays within half of each forward bound of the float64 oracle at every size, channel count
    and background, with and without the scale; the all_outside image is the background in the reference too, and the
    reference gradient is zero exactly there."""
    for H, W in WARP_SIZES:
        worst = 0.0
        for C in WARP_CHANNELS:
            for white in (False, True):
                for scaled in (True, False):
                    r32, r64 = (warp_ref(H, W, C, white, dt, scaled) for dt in (torch.float32, torch.float64))
                    worst = max(worst, maxdiff(r32, r64))
                    assert bool((r64[OUTSIDE] == float(white)).all()), (H, W, C, white)
            g = warp_grad_ref(H, W, C)
            assert not bool(g[OUTSIDE].any()) and (H * W == 1 or all(bool(g[n].any()) for n in range(N_WARP) if n != OUTSIDE)), (H, W, C)
        print('warp %dx%d: float32 vs float64 oracle %.2e (half bound %.1e)' % (H, W, worst, warp_fwd_tol(H, W) / 2))
        assert worst <= warp_fwd_tol(H, W) / 2, (H, W)


def test_handoff_cases_are_well_conditioned():
    """The float32 CPU oracle within half of each bound of the float64 oracle: the forward (1.5e-6 of the largest entry) and
    every gradient (1e-5 of its largest entry), at every shape, with and without the previous image."""
    for shape in HANDOFF_SHAPES:
        for has_prev in (True, False):
            (o32, g32), (o64, g64) = (handoff_ref(*shape, has_prev, dt) for dt in (torch.float32, torch.float64))
            fwd = maxdiff(o32, o64) / float(o64.abs().max())
            grad = {k: maxdiff(g32[k], g64[k]) / float(g64[k].abs().max()) for k in g64}
            print('hand-off %s prev=%d: float32 vs float64 oracle, forward %.2e, gradients %s' % (
                shape, has_prev, fwd, ', '.join('%s %.2e' % kv for kv in grad.items())))
            assert fwd <= HANDOFF_FWD_TOL / 2 and max(grad.values()) <= HANDOFF_GRAD_TOL / 2, (shape, has_prev)


# ------------------------------------------------------------------------------------------------
# 2. pose (GPU)
# ------------------------------------------------------------------------------------------------
def hip_pose(dev, c, proposals=None):
    import nerf_from_image_amd.pose_estimation as pe
    w2c, focal, err = pe.compute_pose_pnp(torch.from_numpy(c['coords']).to(dev), torch.from_numpy(c['masks']).to(dev),
                                          c['proposals'] if proposals is None else proposals)
    assert w2c.dtype == focal.dtype == err.dtype == torch.float32
    return w2c.cpu().numpy(), focal.cpu().numpy(), err.cpu().numpy()


def assert_dummy(tag, b, w2c, focal, err):
    """pose_estimation.py:110-117: a camera looking away from the object, focal 1, error 10 - exactly"""
    assert err[b] == 10.0 and focal[b] == 1.0 and np.array_equal(w2c[b], DUMMY_W2C.astype(np.float32)), (tag, b, w2c[b], focal[b], err[b])


@pytest.mark.gpu
@pytest.mark.parametrize('tag', POSE_EXACT)
def test_pose_recovery_on_exact_data(gpu_device, tag):
    """Exact correspondences: error below 1e-4, the true focal among the proposals, the rotation within 0.5 degrees and the
    translation within 1e-3 of the ground truth - on every image; the images with fewer than 4 foreground pixels carry the
    dummy pose exactly and their neighbours are solved like all others.  `sweep`: with the 64 proposals in reverse order the
    result is the same bits (no two proposals tie)."""
    c = pose_case(tag, 0.0)
    w2c, focal, err = hip_pose(gpu_device, c)
    worst = dict(err=0.0, deg=0.0, t=0.0)
    for b in range(len(err)):
        if b in c['dummy']:
            assert_dummy(tag, b, w2c, focal, err)
            continue
        m = FLIP @ w2c[b].astype(np.float64)
        deg, dt = rot_angle_deg(m[:3, :3], c['R'][b]), float(np.abs(m[:3, 3] - c['t'][b]).max())
        worst = dict(err=max(worst['err'], float(err[b])), deg=max(worst['deg'], deg), t=max(worst['t'], dt))
        assert err[b] < 1e-4 and focal[b] == np.float32(FOCAL), (tag, b, err[b], focal[b])
        assert deg < 0.5 and dt < 1e-3, (tag, b, deg, dt)
        assert np.array_equal(w2c[b, 3], [0, 0, 0, 1])
    print('pose %s exact: error %.2e (bound 1e-4), rotation %.2e deg (0.5), translation %.2e (1e-3)' % (
        tag, worst['err'], worst['deg'], worst['t']))
    if tag == 'sweep':
        again = hip_pose(gpu_device, c, c['proposals'][::-1].copy())
        for a, b_ in zip(again, (w2c, focal, err)):
            assert np.array_equal(a, b_), (a, b_)


@pytest.mark.gpu
@pytest.mark.parametrize('tag', POSE_NOISY)
def test_pose_matches_independent_solver_on_noisy_data(gpu_device, tag):
    """Against orp.compute_pose_pnp: the same focal, np.allclose(err, rtol=1e-4, atol=1e-6), world2cam within 2e-4."""
    c = pose_case(tag, 0.02)
    ref_w2c, ref_f, ref_e = pose_reference(tag, 0.02)
    w2c, focal, err = hip_pose(gpu_device, c)
    print('pose %s noisy: focal %s; error rel %.2e (bound 1e-4); world2cam %.2e (bound 2e-4)' % (
        tag, focal, np.abs(err / ref_e - 1).max(), np.abs(w2c - ref_w2c).max()))
    assert np.array_equal(focal, ref_f.astype(np.float32)), (focal, ref_f)
    assert np.allclose(err, ref_e, rtol=1e-4, atol=1e-6), (err, ref_e)
    assert np.abs(w2c.astype(np.float64) - ref_w2c).max() < 2e-4


@pytest.mark.gpu
def test_pose_mask_threshold_is_strict_and_dummies_match_the_oracle(gpu_device):
    """`mixed` once more, against the oracle fed with mask > 0.5: the same images come back as dummies and the same focal is
    chosen elsewhere - a mask value of exactly 0.5 is background (with it as foreground image 3 would be solved over all 240
    pixels, most of them with coordinates (0, 0, 0))."""
    c = pose_case('mixed', 0.0)
    ref_w2c, ref_f, ref_e = pose_reference('mixed', 0.0)
    w2c, focal, err = hip_pose(gpu_device, c)
    assert [b for b in range(4) if ref_e[b] == 10.0] == list(c['dummy'])
    assert np.array_equal(focal, ref_f.astype(np.float32)), (focal, ref_f)
    for b in c['dummy']:
        assert_dummy('mixed', b, w2c, focal, err)
        assert np.array_equal(w2c[b].astype(np.float64), ref_w2c[b])
    assert err[3] < 1e-4 and err[0] < 1e-4, err


# ------------------------------------------------------------------------------------------------
# 3. image metrics (GPU)
# ------------------------------------------------------------------------------------------------
def layouts(t):
    """[B,3,H,W] and the same values as [B,H,W,3]"""
    return (('BCHW', t), ('BHWC', t.permute(0, 2, 3, 1).contiguous()))


@pytest.mark.gpu
@pytest.mark.parametrize('B,H,W', METRIC_SHAPES)
def test_image_metrics_against_float64(gpu_device, B, H, W):
    """PSNR within 2e-4 dB of orn.psnr on float64 inputs, in both layouts, exactly 60.0 for an image equal to its target; IoU
    torch.equal with orn.iou for [B,H,W] and [B,1,H,W] masks; psnr_and_iou returns the bits of the two single calls; a call
    for one metric returns None for the other."""
    from nerf_from_image_amd import metrics, ops
    dev = gpu_device
    c = metric_case(B, H, W)
    mp, mr = c['mask_pred'].to(dev), c['mask_real'].to(dev)
    iou = metrics.iou(mp, mr, reduction='none')
    assert iou.shape == (B,) and torch.equal(iou.cpu(), c['iou']), (iou, c['iou'])
    assert torch.equal(metrics.iou(mp.unsqueeze(1), mr.unsqueeze(1), reduction='none'), iou)
    assert float(metrics.iou(mp, mr)) == pytest.approx(float(c['iou'].mean()), abs=1e-6)
    worst = 0.0
    for (name, p), (_, t) in zip(layouts(c['pred']), layouts(c['target'])):
        p, t = p.to(dev), t.to(dev)
        per = metrics.psnr(p, t, reduction='none')
        assert per.shape == (B,)
        worst = max(worst, maxdiff(per.cpu(), c['psnr64']))
        assert maxdiff(per.cpu(), c['psnr64']) <= PSNR_TOL, (name, per, c['psnr64'])
        for b, same in enumerate(c['identical']):
            assert not same or float(per[b]) == 60.0, (name, b, per)
        assert abs(float(metrics.psnr(p, t)) - float(c['psnr64'].mean())) <= PSNR_TOL
        both = metrics.psnr_and_iou(p, t, mp, mr)
        assert torch.equal(both[0], per) and torch.equal(both[1], iou), name
        only_psnr, none_iou, flag = ops.image_metrics(pred=p, target=t)
        assert none_iou is None and torch.equal(only_psnr, per) and int(flag) == 0
    none_psnr, only_iou, flag = ops.image_metrics(mask_pred=mp, mask_real=mr)
    assert none_psnr is None and torch.equal(only_iou, iou) and int(flag) == 0
    print('metrics %s: PSNR within %.2e dB of float64 (bound %.0e), %s' % ((B, H, W), worst, PSNR_TOL, c['psnr64'].tolist()))


@pytest.mark.gpu
def test_mask_threshold_is_strict(gpu_device):
    """A mask of exactly 0.5 is empty, the next float above it is full; two empty masks give exactly 1.0."""
    from nerf_from_image_amd import metrics
    B, H, W = EDGE_SHAPE
    half, above = torch.full((B, H, W), float(HALF)), torch.full((B, H, W), float(ABOVE_HALF))
    split = half.clone()
    split[:, :, W // 2:] = float(ABOVE_HALF)           # 0.5 on one side, the next float on the other
    n_right = H * (W - W // 2)
    for a, b, inter, union in ((half, above, 0, H * W), (above, half, 0, H * W), (split, above, n_right, H * W),
                               (above, split, n_right, H * W), (split, split, n_right, n_right), (half, split, 0, n_right),
                               (above, above, H * W, H * W)):
        got = metrics.iou(a.to(gpu_device), b.to(gpu_device), reduction='none').cpu()
        want = (torch.tensor(float(inter)) + 1e-6) / (torch.tensor(float(union)) + 1e-6)
        assert torch.equal(got, orn.iou(a, b)) and torch.equal(got, want.expand(B)), (inter, union, got)
    for empty in (half, torch.zeros(B, H, W), torch.full((B, H, W), -0.05)):
        got = metrics.iou(empty.to(gpu_device), torch.zeros(B, H, W).to(gpu_device), reduction='none').cpu()
        assert torch.equal(got, torch.ones(B)), got


BAD_VALUES = {'1.1': np.float32(1.1), '-0.1': np.float32(-0.1), 'nan': np.float32('nan')}
ALMOST_BAD = {'below 1.1': np.nextafter(np.float32(1.1), np.float32(0)), 'above -0.1': np.nextafter(np.float32(-0.1), np.float32(0))}


@pytest.mark.gpu
def test_range_check_at_its_limits_and_at_the_last_element(gpu_device):
    """lib/metrics.py:22-27: -0.1 < v < 1.1.  One element of exactly float32(1.1), float32(-0.1) or NaN - the last element of
    the last image, where a loop that stops early would not look - in pred, target or either mask fails the check; the next
    floats towards zero do not; with check_range=False there is no flag and the call succeeds."""
    from nerf_from_image_amd import metrics, ops
    dev = gpu_device
    c = metric_case(*EDGE_SHAPE)
    names = ('pred', 'target', 'mask_pred', 'mask_real')
    clean = {k: c[k] for k in names}

    def with_last(which, value):
        t = dict(clean)
        t[which] = clean[which].clone()
        t[which].view(-1)[-1] = float(value)
        assert float(t[which][-1].flatten()[-1]) == float(value) or value != value
        return {k: v.to(dev) for k, v in t.items()}
    for which in names:
        call = ((lambda t: metrics.psnr(t['pred'], t['target'], reduction='none')) if which in ('pred', 'target') else
                (lambda t: metrics.iou(t['mask_pred'], t['mask_real'], reduction='none')))
        for label, value in BAD_VALUES.items():
            with pytest.raises(AssertionError, match='Range check'):
                call(with_last(which, value))
            t = with_last(which, value)
            with pytest.raises(AssertionError, match='Range check'):
                metrics.psnr_and_iou(t['pred'], t['target'], t['mask_pred'], t['mask_real'])
            if which in ('pred', 'target'):      # the other layout: the element is the last one there too
                with pytest.raises(AssertionError, match='Range check'):
                    metrics.psnr(t['pred'].permute(0, 2, 3, 1).contiguous(), t['target'].permute(0, 2, 3, 1).contiguous())
        for label, value in ALMOST_BAD.items():
            got = call(with_last(which, value))
            assert bool(torch.isfinite(got).all()), (which, label, got)
    t = with_last('pred', BAD_VALUES['1.1'])
    t['mask_real'].view(-1)[-1] = float('nan')
    psnr, iou, flag = ops.image_metrics(t['pred'], t['target'], t['mask_pred'], t['mask_real'], check_range=False)
    assert flag is None and psnr.shape == iou.shape == (EDGE_SHAPE[0],) and bool(torch.isfinite(psnr).all())
    psnr, iou, flag = ops.image_metrics(t['pred'], t['target'], t['mask_pred'], t['mask_real'])
    assert int(flag) == 1


# ------------------------------------------------------------------------------------------------
# 4. warp (GPU)
# ------------------------------------------------------------------------------------------------
def warp_tform(dev, scaled=True):
    return WARP_ROT.to(dev), WARP_SCALE.to(dev) if scaled else None, WARP_TRANS.to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize('H,W', WARP_SIZES)
def test_warp_forward_against_float64(gpu_device, H, W):
    """ops.affine_warp against orn.warp_images in float64 for 1, 8, 9 and 17 channels and both backgrounds, seven transforms
    per call, and once more with scale = NULL; the image whose samples all fall outside is the background exactly."""
    from nerf_from_image_amd import ops
    dev = gpu_device
    tol, worst = warp_fwd_tol(H, W), 0.0
    for C in WARP_CHANNELS:
        x = warp_case(H, W, C)[0].to(dev)
        for white in (False, True):
            for scaled in (True, False):
                got = ops.affine_warp(x, *warp_tform(dev, scaled), white).cpu()
                ref = warp_ref(H, W, C, white, torch.float64, scaled)
                assert got.shape == ref.shape
                per_image = (got.double() - ref).abs().flatten(1).max(dim=1)[0]
                worst = max(worst, float(per_image.max()))
                assert float(per_image.max()) <= tol, (C, white, scaled, dict(zip(NAMES, per_image.tolist())))
                assert torch.equal(got[OUTSIDE], torch.full((C, H, W), float(white))), (C, white, scaled)
    print('warp forward %dx%d: max err %.3e (bound %.0e)' % (H, W, worst, tol))


@pytest.mark.gpu
@pytest.mark.parametrize('H,W', WARP_SIZES)
def test_warp_backwards_against_float64_autograd(gpu_device, H, W):
    """nfi_affine_warp_bwd and nfi_affine_warp_bwd_ordered against float64 autograd of the oracle, per image within 1e-4 of
    that image's largest gradient entry, zeros where every sample falls outside; both background flags (the flag does not
    enter the adjoint).  The ordered entry: three launches are torch.equal, and with 9 and 17 channels every channel's
    gradient is, bit for bit, the ordered gradient of that channel run alone - the kernel adds per channel in the same
    window order whichever pass of 8 the channel falls into."""
    from nerf_from_image_amd import ops
    dev = gpu_device
    worst = {False: 0.0, True: 0.0}
    for C in WARP_CHANNELS:
        y = warp_case(H, W, C)[1].to(dev)
        ref = warp_grad_ref(H, W, C)
        scale = ref.abs().flatten(1).max(dim=1)[0]
        for ordered in (False, True):
            for white in (False, True):
                got = ops.affine_warp_bwd(y, *warp_tform(dev), white, ordered=ordered)
                err = (got.cpu().double() - ref).abs().flatten(1).max(dim=1)[0]
                worst[ordered] = max(worst[ordered], float((err / scale.clamp_min(1e-30)).max()))
                assert bool((err <= WARP_GRAD_TOL * scale).all()), (C, ordered, white, dict(zip(NAMES, zip(err.tolist(), scale.tolist()))))
                assert not bool(got[OUTSIDE].any()), (C, ordered, white)
        first = ops.affine_warp_bwd(y, *warp_tform(dev), False, ordered=True)
        for launch in (1, 2):
            assert torch.equal(ops.affine_warp_bwd(y, *warp_tform(dev), False, ordered=True), first), (C, launch)
        if C > 8:
            for ch in range(C):
                alone = ops.affine_warp_bwd(y[:, ch:ch + 1].contiguous(), *warp_tform(dev), False, ordered=True)
                assert torch.equal(alone[:, 0], first[:, ch]), (C, ch)
    print('warp backward %dx%d: max err / largest entry, atomic %.3e, ordered %.3e (bound %.0e)' % (
        H, W, worst[False], worst[True], WARP_GRAD_TOL))


# ------------------------------------------------------------------------------------------------
# 5. hand-off (GPU)
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('has_prev', [True, False], ids=['prev', 'no_prev'])
@pytest.mark.parametrize('B,Cin,R', HANDOFF_SHAPES)
def test_handoff_forward_against_float64(gpu_device, B, Cin, R, has_prev):
    """ops.torgb_texels against orn.torgb_upsample_add in float64: within 3e-6 of the reference's largest entry, written
    channels-last."""
    from nerf_from_image_amd import ops
    t = {k: v.to(gpu_device) for k, v in handoff_case(B, Cin, R).items()}
    ref, _ = handoff_ref(B, Cin, R, has_prev, torch.float64)
    out = ops.torgb_texels(t['x'], t['s'], t['w'], t['bias'], t['prev'] if has_prev else None)
    assert out.shape == (B, 96, R, R) and out.is_contiguous(memory_format=torch.channels_last)
    err, scale = maxdiff(out.cpu(), ref), float(ref.abs().max())
    print('hand-off forward %s prev=%d: max err %.3e of %.3e (bound %.3e)' % ((B, Cin, R), has_prev, err, scale, HANDOFF_FWD_TOL * scale))
    assert err <= HANDOFF_FWD_TOL * scale


@pytest.mark.gpu
@pytest.mark.parametrize('want_weight', [True, False], ids=['weight', 'no_weight'])
@pytest.mark.parametrize('has_prev', [True, False], ids=['prev', 'no_prev'])
@pytest.mark.parametrize('B,Cin,R', HANDOFF_SHAPES)
def test_handoff_atomic_backward_against_float64(gpu_device, B, Cin, R, has_prev, want_weight):
    """ops.torgb_texels_bwd(ordered=False): every gradient - the style, weight and bias sums of float atomics among them -
    within 2e-5 of the largest entry of float64 autograd of the oracle."""
    from nerf_from_image_amd import ops
    t = {k: v.to(gpu_device) for k, v in handoff_case(B, Cin, R).items()}
    _, ref = handoff_ref(B, Cin, R, has_prev, torch.float64)
    got = ops.torgb_texels_bwd(t['up'], t['x'], t['s'], t['w'], t['prev'] if has_prev else None, want_weight=want_weight, ordered=False)
    keys = ['g_x', 'g_styles'] + (['g_weight', 'g_bias'] if want_weight else []) + (['g_previous_image'] if has_prev else [])
    assert sorted(got) == sorted(keys)
    for k in keys:
        assert got[k].shape == ref[k].shape, k
        err, scale = maxdiff(got[k].cpu(), ref[k]), float(ref[k].abs().max())
        print('hand-off backward %s prev=%d %s: max err %.3e of %.3e (bound %.3e)' % ((B, Cin, R), has_prev, k, err, scale, HANDOFF_GRAD_TOL * scale))
        assert err <= HANDOFF_GRAD_TOL * scale, (k, err, scale)
