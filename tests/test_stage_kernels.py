"""The stand-alone per-ray stage entry points at the sizes and inputs where their kernels change path.

What the nerf_utils drop-in, the staged render path and the training backward call - nfi_raygen, nfi_near_far,
nfi_stratified_points, nfi_points_on_rays, nfi_ray_weights, nfi_sample_pdf, nfi_resample, nfi_composite_fwd and the four
backward entries - is held to the oracle here at template and kernel switches (both sides), in grid-stride passes, with
idle waves behind the last ray, on degenerate inputs (exact zeros in directions, tied depths, one-hot pdfs, u on the cdf's
own entries) and through wrappers that must refuse malformed arguments before they launch.

Bounds (the suite's own for the same quantities):
  origins, near / far / hit on identical inputs, stratified depths, query points, searchsorted indices on the kernel's own
  cdf, sorted depths, permutation: bit-exact;  ray directions 2e-7;  weights, smoothed weights, cdf 1e-6;  fine depths /
  samples, rgb / depth / mask / extra maps 1e-5;  gradients: rel_close of test_hip_backward.py (2e-4 of the gradient's
  scale);  the fused render 1e-4 (ATOL of test_hip_parity.py).
References: oracle/nfi_oracle.py - in float32 where bit equality is demanded, in float64 elsewhere.  The CPU tests at the
top assert, for the inputs the GPU tests use (the shared, cached case builders below), that the float32 oracle is within
HALF of the bound of the float64 oracle, so a GPU failure cannot be blamed on the input.  Two things are outside that
rule and say so where they are asserted: unit ray directions (float32 normalisation alone is 1.07e-7 from float64;
asserted at UNIT_DIR_F32 = 1.49e-7, and held to the float32 oracle on the GPU) and the quantities compared bit for bit (float32 oracle;
the stratified / query-point inputs and the hand-built rays have no float64 counterpart to be conditioned against).

Forward stage tests call the C entry points directly (_lib.call_struct) into caller-allocated buffers that carry GUARD
sentinel rows behind the last ray; N runs over 1, 2, 3, 5, 9 so that the last block of four waves has one to three idle
waves, and the guard must come back untouched.
"""
import functools
import re
import struct

import pytest
import torch

from conftest import load_golden
from parity_util import hip_render, oracle_render
from test_hip_backward import oracle_merge_composite, rel_close
from test_hip_parity import ATOL, close, exact
from nerf_from_image_amd import _lib, ops
from oracle import nfi_oracle as orc

DIR_TOL = 2e-7
W_TOL = 1e-6        # weights, smoothed weights, cdf
MAP_TOL = 1e-5      # fine depths / samples, composited maps
GRAD_TOL = 2e-4     # rel_close's default
# What float32 F.normalize itself leaves between the float32 and the float64 oracle at a component of magnitude 1: the sum
# of squares (three roundings, halved by the root), the square root and the division - 2.5 roundings of 2^-24 = 1.49e-7.
# It does not depend on the camera (measured 1.07e-7 over the ~3 000 rays of the camera families, 1.39e-7 over the 264 500
# of the large case), and it is more than half of 2e-7: so unit directions are held to the FLOAT32 oracle on the GPU, the
# reference tests/test_hip_parity.py has for that bound, and the conditioning tests assert this figure for them.
UNIT_DIR_F32 = 2.5 * 2.0 ** -24

NS = (1, 2, 3, 5, 9)
NMAX = max(NS)
GUARD = 4
FAMILIES = ('zero', 'uniform', 'wall', 'sparse', 'thin')
PDF_KINDS = ('random', 'zero', 'onehot', 'smoothed')

WEIGHT_S = (2, 3, 63, 64, 65, 127, 128, 129, 257, 511, 512)
PDF_M = (2, 3, 8, 9, 63, 64, 65, 127, 128)
PDF_K = (1, 63, 64, 65, 128)
PDF_MK = [(m, k) for m in PDF_M for k in PDF_K if m != k + 1]
RESAMPLE_S = (4, 5, 8, 9, 63, 64, 65, 66, 72, 127, 128)
# without 'thin': weights of 1e-3 leave a pdf of 0.01 floors, where the reference's own 3e-8 of weight error is 5e-7 of cdf
RESAMPLE_FAMILIES = ('zero', 'uniform', 'wall', 'sparse')
COMPOSITE_LISTS = [(1, 1), (3, 5), (127, 1), (128, 1), (1, 128), (64, 65), (100, 128), (128, 128),
                   (2, 0), (128, 0), (129, 0), (256, 0), (257, 0), (512, 0)]
EXTRAS = (0, 1, 14, 33)
STRATIFIED_S = (1, 3, 127, 512)


def seed_of(*parts):
    """A seed that does not depend on Python's string hashing."""
    s = 17
    for p in parts:
        for ch in str(p):
            s = (s * 131 + ord(ch)) % 2147483629
    return s


def rng(*parts):
    return torch.Generator().manual_seed(seed_of(*parts))


# ------------------------------------------------------------------------------------------------
# input families (CPU, float32) and their references, computed once and shared
# ------------------------------------------------------------------------------------------------
def directions(n, g):
    """non-unit directions, 0.5 <= |d| <= 2"""
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    return d * (0.5 + 1.5 * torch.rand(n, 1, generator=g))


def depths(n, s, g):
    """ascending depths in [0.5, 2.5]"""
    return torch.sort(torch.rand(n, s, generator=g) * 2 + 0.5, dim=-1)[0]


def sigma_family(kind, n, s, g):
    r = torch.rand(n, s, generator=g)
    if kind == 'zero':
        return torch.zeros(n, s)
    if kind == 'uniform':
        return r * 1e4
    if kind == 'wall':
        out = torch.zeros(n, s)
        out[:, s // 2:] = 1e6
        return out
    if kind == 'sparse':
        return r * 8 * (torch.rand(n, s, generator=g) > 0.7)
    if kind == 'thin':
        return r * 0.05
    raise KeyError(kind)


def sigma_rows(n, s, g):
    """one family per row (sparse, uniform, thin, wall, zero, sparse, ...): every family in every batch"""
    order = ('sparse', 'uniform', 'thin', 'wall', 'zero')
    return torch.cat([sigma_family(order[i % 5], 1, s, g) for i in range(n)], dim=0)


@functools.lru_cache(maxsize=None)
def weights_case(kind, S):
    g = rng('weights', kind, S)
    c = dict(sigma=sigma_family(kind, NMAX, S, g), rd=directions(NMAX, g), t=depths(NMAX, S, g))
    for name, dt in (('w32', torch.float32), ('w64', torch.float64)):
        c[name] = orc.ray_weights(c['sigma'].to(dt), c['rd'].to(dt), c['t'].to(dt))
    return c


@functools.lru_cache(maxsize=None)
def composite_case(na, nb):
    """N = 9 rays.  Two lists: a ascending, b in any order; ray 0: b[0] equals an entry of a (and b[1] another one), ray 1:
    two equal entries of b, ray 2: all depths equal, rays 3..: every fourth entry of b copies an entry of a."""
    g = rng('composite', na, nb)
    c = dict(rd=directions(NMAX, g), t_a=depths(NMAX, na, g), s_a=sigma_rows(NMAX, na, g),
             c_a=torch.rand(NMAX, na, 3, generator=g) * 2 - 1, e_a=torch.rand(NMAX, na, max(EXTRAS), generator=g),
             t_b=None, s_b=None, c_b=None, e_b=None)
    if nb:
        t_b = torch.rand(NMAX, nb, generator=g) * 2 + 0.5
        t_b[0, 0] = c['t_a'][0, na // 2]
        if nb > 1:
            t_b[0, 1] = c['t_a'][0, 0]
            t_b[1, nb - 1] = t_b[1, 0]
        c['t_a'][2] = 1.0
        t_b[2] = 1.0
        for r in range(3, NMAX):
            idx = torch.randint(0, na, (len(range(0, nb, 4)),), generator=g)
            t_b[r, 0::4] = c['t_a'][r, idx]
        c.update(t_b=t_b, s_b=sigma_rows(NMAX, nb, g), c_b=torch.rand(NMAX, nb, 3, generator=g) * 2 - 1,
                 e_b=torch.rand(NMAX, nb, max(EXTRAS), generator=g))
    return c


@functools.lru_cache(maxsize=None)
def composite_ref(na, nb, white, n_extra, dt):
    """merge (torch.sort, stable, on the float32 depths) + orc.composite in `dt`"""
    c = composite_case(na, nb)
    two = nb > 0
    t = torch.cat((c['t_a'], c['t_b']), -1) if two else c['t_a']
    s = (torch.cat((c['s_a'], c['s_b']), -1) if two else c['s_a']).to(dt)
    col = (torch.cat((c['c_a'], c['c_b']), -2) if two else c['c_a']).to(dt)
    e = None
    if n_extra:
        e = (torch.cat((c['e_a'], c['e_b']), -2) if two else c['e_a'])[..., :n_extra].to(dt)
    perm = torch.arange(na + nb).expand(NMAX, -1).contiguous()
    if two:
        t, perm = torch.sort(t, dim=-1, stable=True)
        s = s.gather(-1, perm)
        col = col.gather(-2, perm.unsqueeze(-1).expand(*perm.shape, 3))
        if e is not None:
            e = e.gather(-2, perm.unsqueeze(-1).expand(*perm.shape, n_extra))
    rgb, depth, acc, ex, w = orc.composite(s, col, c['rd'].to(dt), t.to(dt), e, white)
    return dict(rgb=rgb, depth=depth, mask=acc, extra=ex, weights=w, perm=perm, depth_sorted=t)


def pdf_weights(kind, n, m, g):
    w = torch.rand(n, m - 1, generator=g)
    if kind == 'random':
        return w * 0.75 + 0.25          # no bin so thin that the reference's own rounding moves a sample by 5e-6
    if kind == 'zero':
        return torch.zeros(n, m - 1)
    if kind == 'onehot':
        out = torch.zeros(n, m - 1)
        out[torch.arange(n), torch.randint(0, m - 1, (n,), generator=g)] = 1.0
        return out
    if kind == 'smoothed':
        return orc.smooth_weights(0.2 * w * (torch.rand(n, m - 1, generator=g) > 0.5))
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def pdf_case(kind, M, K):
    """bins [9,M], weights [9,M-1]; u 'dense' [9,K]: per row drawn from 0, 1 - 2^-24, 1.0, the M entries of the row's own
    (float32 oracle) cdf and K uniform numbers; u 'lin': the one linspace(0,1,K) row every randomize=False call broadcasts."""
    g = rng('pdf', kind, M, K)
    bins = torch.linspace(1.0, 2.0, M) + (torch.rand(NMAX, M, generator=g) - 0.5) * (0.6 / (M - 1))    # ascending
    w = pdf_weights(kind, NMAX, M, g)
    lin = torch.linspace(0.0, 1.0, steps=K)
    _, _, c32 = orc.inverse_cdf(bins, w, lin.expand(NMAX, K))
    dense = torch.empty(NMAX, K)
    for r in range(NMAX):
        pool = torch.cat((torch.tensor([0.0, 1.0 - 2.0 ** -24, 1.0]), c32[r], torch.rand(K, generator=g)))
        dense[r] = pool[(r * K + torch.arange(K)) % pool.numel()]
    c = dict(bins=bins, weights=w, dense=dense, lin=lin)
    for mode, u in (('dense', dense), ('lin', lin.expand(NMAX, K))):
        for name, dt in (('32', torch.float32), ('64', torch.float64)):
            smp, inds, cdf = orc.inverse_cdf(bins.to(dt), w.to(dt), u.to(dt))
            c[mode + name] = dict(samples=smp, inds=inds, cdf=cdf)
    return c


def interpolate_on_cdf(bins, cdf, u):
    """orc.inverse_cdf's search, gather and interpolation (float32) on a GIVEN cdf: what the kernel must return for the cdf
    it wrote itself, whichever side of the `den < 1e-5` switch a bin of that cdf falls on."""
    cdf, u = cdf.contiguous(), u.contiguous()
    inds = torch.searchsorted(cdf, u, right=True)
    lo, hi = (inds - 1).clamp(min=0), inds.clamp(max=cdf.shape[-1] - 1)
    c_lo, c_hi = cdf.gather(-1, lo), cdf.gather(-1, hi)
    b_lo, b_hi = bins.gather(-1, lo), bins.gather(-1, hi)
    den = c_hi - c_lo
    den = torch.where(den < 1e-5, torch.ones_like(den), den)
    return b_lo + ((u - c_lo) / den) * (b_hi - b_lo), inds


@functools.lru_cache(maxsize=None)
def resample_case(kind, S):
    g = rng('resample', kind, S)
    c = dict(sigma=sigma_family(kind, NMAX, S, g), rd=directions(NMAX, g), t=depths(NMAX, S, g),
             dense=torch.rand(NMAX, S, generator=g), lin=torch.linspace(0.0, 1.0, steps=S))
    for mode, u in (('dense', c['dense']), ('lin', c['lin'].expand(NMAX, S))):
        for name, dt in (('32', torch.float32), ('64', torch.float64)):
            sg, rd, t = c['sigma'].to(dt), c['rd'].to(dt), c['t'].to(dt)
            w = orc.ray_weights(sg, rd, t)
            ws = orc.smooth_weights(w.float()).to(dt) if dt == torch.float32 else _smooth64(w)
            mid = .5 * (t[..., 1:] + t[..., :-1])
            fine, inds, cdf = orc.inverse_cdf(mid, ws[..., 1:-1], u.to(dt))
            c[mode + name] = dict(weights=w, smooth=ws, cdf=cdf, inds=inds, fine=fine)
    return c


def _smooth64(w):
    """orc.smooth_weights without its cast to float32 (the float64 reference)"""
    F = torch.nn.functional
    return F.avg_pool1d(F.max_pool1d(w.unsqueeze(1), 2, 1, padding=1), 2, 1).squeeze(1) + 0.01


def maxdiff(a, b):
    return float((a.double() - b.double()).abs().max()) if a.numel() else 0.0


# ------------------------------------------------------------------------------------------------
# cameras
# ------------------------------------------------------------------------------------------------
# scene cube of the camera tests: no pixel grid used below puts a parallel ray on a face plane
def camera_range(kind):
    return 1.3 if kind == 'ortho_axes' else 0.7      # (the plain orthographic 1 x N images lie at |y| = 1)


CAMERA_SHAPES = ((1, 8), (8, 1), (1, 7), (6, 8), (5, 7))
CAMERA_KINDS = ('persp_identity', 'persp_axes', 'persp_center', 'persp_bbox', 'persp_center_bbox', 'ortho_axes',
                'ortho_bbox')


def axis_views(w=1.0):
    """six cam2world matrices [6,4,4] looking along +-x, +-y, +-z at the origin from distance 2: every entry of the rotation
    is an exact 0, -0 or +-1; w: the homogeneous scale cam2world[3,3] (a scalar or six values)"""
    out = torch.zeros(6, 4, 4)
    i = 0
    for axis in range(3):
        for sign in (1.0, -1.0):
            fwd, up = torch.zeros(3), torch.zeros(3)
            fwd[axis], up[(axis + 1) % 3] = sign, 1.0
            right = torch.linalg.cross(fwd, up)
            out[i, :3, :3] = torch.stack((right, up, -fwd), dim=1)
            out[i, :3, 3] = -2.0 * fwd
            i += 1
    out[:, 3, 3] = torch.as_tensor(w)
    return out


def camera(kind):
    """dict(cam2world, focal, bbox, center) of one camera family (float32)"""
    # the narrow cameras always hit, the wide ones also miss; |raw direction components| <= 1, where 2e-7 is more than an ulp
    focal6 = torch.tensor([1.0, 0.75, 1.0, 0.75, 1.0, 0.75])
    bbox6 = torch.tensor([[[-1.0, -1.0], [2.0, 2.0]], [[-0.5, -0.25], [1.0, 0.5]]]).repeat(3, 1, 1)
    center6 = torch.tensor([[0.5, 0.5], [0.46875, 0.53125], [0.515625, 0.5]]).repeat(2, 1)
    c = dict(cam2world=axis_views(), focal=focal6, bbox=None, center=None)
    if kind == 'persp_identity':
        eye = torch.eye(4).repeat(2, 1, 1)
        eye[1, 2, 3] = 2.0
        c.update(cam2world=eye, focal=torch.tensor([1.0, 0.75]))
    elif kind == 'persp_center':
        c.update(center=center6)
    elif kind == 'persp_bbox':
        c.update(bbox=bbox6)
    elif kind == 'persp_center_bbox':
        c.update(bbox=bbox6, center=center6)
    elif kind == 'ortho_axes':
        c.update(cam2world=axis_views(torch.tensor([1.25, 1.25, 1.25, 0.5, 0.5, 0.5])), focal=None)
    elif kind == 'ortho_bbox':
        c.update(cam2world=axis_views(1.25), focal=None, bbox=bbox6)
    elif kind != 'persp_axes':
        raise KeyError(kind)
    return c


def to_(c, dt=None, dev=None):
    return {k: (v if v is None else v.to(dtype=dt, device=dev)) for k, v in c.items()}


@functools.lru_cache(maxsize=None)
def camera_rays(kind, H, W, dt=torch.float32):
    c = to_(camera(kind), dt)
    ro, rd = orc.ray_bundle(H, W, c['focal'], c['cam2world'], c['bbox'], c['center'])
    return ro.contiguous(), rd, orc.unit_dirs(rd)


def hand_built_rays():
    """rays with exact 0 and -0 components against the cube [-0.5, 0.5]^3: axis-parallel through the cube, from inside it
    (near < 0: the 0.1 clamp), axis-parallel beside it (the infinities decide), grazing an edge (far - near < 1e-3) and
    plain misses.  Parallel rays stay off the face planes."""
    e = 2e-4
    ro = torch.tensor([[0.0, 0.0, 2.0], [0.1, -0.2, 2.0], [0.1, 0.2, 0.3], [0.7, 0.0, 2.0], [-0.5 - e, 0.0, 1.5],
                       [3.0, 3.0, 3.0], [-0.0, 2.0, -0.0], [0.25, 0.25, -0.25], [2.0, 0.1, 0.6], [0.0, 0.0, 0.0]])
    rd = torch.tensor([[0.0, 0.0, -1.0], [-0.0, 0.0, -1.0], [0.0, -0.0, 1.0], [0.0, 0.0, -1.0], [1.0, 0.0, -1.0],
                       [0.0, 0.0, 1.0], [0.0, -1.0, -0.0], [-0.0, -0.0, -2.0], [-1.0, -0.0, 0.0], [0.5, -0.0, 0.0]])
    return ro, rd, 0.5


def ordered_key(x):
    b = struct.unpack('<I', struct.pack('<f', float(x)))[0]
    return b ^ (0xFFFFFFFF if b >> 31 else 0x80000000)


LARGE_NEAR_FAR = 70001       # > kSlabBlocks * 256 = 65 536: rays from there on belong to the grid-stride pass


@functools.lru_cache(maxsize=None)
def large_near_far_case():
    """70 001 rays against the cube [-0.5, 0.5]^3 from outside it.  Rays below 65 536: from radius 3 at points of the cube
    (hits, near >= 2.1, far <= 3.9) or past it (misses).  In the tail: more of the same, the ray with the smallest near
    (from distance 1 along an axis) and the one with the largest far (from distance 6)."""
    g = rng('large near far')
    n = LARGE_NEAR_FAR
    ro = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1) * 3
    target = (torch.rand(n, 3, generator=g) - 0.5) * torch.where(torch.rand(n, 1, generator=g) > 0.4, 0.9, 6.0)
    rd = torch.nn.functional.normalize(target - ro, dim=-1)
    ro[n - 1], rd[n - 1] = torch.tensor([0.05, 1.0, -0.1]), torch.tensor([0.0, -1.0, 0.0])
    ro[n - 2], rd[n - 2] = torch.tensor([6.0, 0.1, 0.2]), torch.tensor([-1.0, 0.0, -0.0])
    near, far, hit = orc.near_far(ro, rd, 0.5)
    odd = hit & ((near <= 0.1) | (far - near <= 2e-3))      # the cube behind the origin, or grazed: aim those at the centre
    rd[odd] = torch.nn.functional.normalize(-ro[odd], dim=-1)
    near, far, hit = orc.near_far(ro, rd, 0.5)
    return ro, rd, near, far, hit


LARGE_RAYGEN = (5, 230, 230)     # 264 500 rays > kRayBlocks * 256 = 262 144


@functools.lru_cache(maxsize=None)
def large_raygen_case():
    """five of the axis views, each from its own position, focal lengths and principal points as in camera(): raw direction
    components stay at or below 1, where 2e-7 is more than an ulp (random rotations and wide cameras put 1.5e-7 between the
    float32 and the float64 oracle)"""
    g = rng('large raygen')
    B = LARGE_RAYGEN[0]
    cam = axis_views()[:B].clone()
    cam[:, :3, 3] = torch.randn(B, 3, generator=g)
    return dict(cam2world=cam, focal=torch.tensor([1.0, 2.0, 1.0, 2.0, 1.0]), bbox=None,
                center=0.5 + (torch.rand(B, 2, generator=g) - 0.5) * 0.0625)


def large_raygen_rays(dt=torch.float32):
    B, H, W = LARGE_RAYGEN
    c = to_(large_raygen_case(), dt)
    ro, rd = orc.ray_bundle(H, W, c['focal'], c['cam2world'], None, c['center'])
    return ro.contiguous(), rd, orc.unit_dirs(rd)


def render_case(kind):
    """The planes and decoder of a golden case under an axis-aligned camera: 2 x 6 x 8 pixels, S = 16, fine pass."""
    meta, t = load_golden('persp_white_fine_rand')
    H, W, S, B = 6, 8, 16, 2
    g = rng('render', kind)
    meta = dict(meta, H=H, W=W, S=S, fine=True, ortho=kind == 'ortho', randomize=True, bbox=False)
    t = {k: v for k, v in t.items() if not k.startswith('ref_')}
    cam = torch.eye(4).repeat(B, 1, 1)
    if kind == 'persp':
        cam[1, 2, 3] = 1.5                         # camera 0: THE identity pose, inside the cube; camera 1: in front of it
    else:
        cam[0, 2, 3] = 2.0
        cam[1] = axis_views()[1]                   # along -x ... +x
        cam[:, 3, 3] = 1.25
        del t['focal']
    t.update(cam2world=cam, noise_coarse=torch.rand(B, H, W, S, generator=g), noise_fine=torch.rand(B * H * W, S, generator=g))
    return meta, t


# ------------------------------------------------------------------------------------------------
# 1. the inputs are well conditioned for the reference (CPU)
# ------------------------------------------------------------------------------------------------
def test_weight_and_composite_inputs_are_well_conditioned():
    """float32 oracle within half the bound of the float64 oracle: weights (5e-7) for every sigma family at every S of the
    ray_weights test, weights / maps / extra maps (5e-7 / 5e-6) for every case of the composite test."""
    worst_w = worst_m = 0.0
    for kind in FAMILIES:
        for S in WEIGHT_S:
            c = weights_case(kind, S)
            worst_w = max(worst_w, maxdiff(c['w32'], c['w64']))
    for na, nb in COMPOSITE_LISTS:
        for white in (True, False):
            for n_extra in EXTRAS:
                r32, r64 = (composite_ref(na, nb, white, n_extra, dt) for dt in (torch.float32, torch.float64))
                assert torch.equal(r32['perm'], r64['perm'])
                worst_w = max(worst_w, maxdiff(r32['weights'], r64['weights']))
                worst_m = max([worst_m] + [maxdiff(r32[k], r64[k]) for k in ('rgb', 'depth', 'mask')] +
                              ([maxdiff(r32['extra'], r64['extra'])] if n_extra else []))
    print('float32 vs float64 oracle: weights %.2e (half bound %.1e), maps %.2e (half bound %.1e)' % (
        worst_w, W_TOL / 2, worst_m, MAP_TOL / 2))
    assert worst_w <= W_TOL / 2 and worst_m <= MAP_TOL / 2


def test_pdf_and_resample_inputs_are_well_conditioned():
    """float32 oracle within half the bound of the float64 oracle for every case of the sample_pdf and resample tests: cdf,
    weights, smoothed weights 5e-7; samples / fine depths 5e-6 - except the samples of the one-hot rows, whose empty bins sit on
    the reference's own `den < 1e-5` switch (those are held to the kernel's own cdf instead, see the GPU test).  With
    uniform u no searchsorted index differs between the two precisions (u placed ON cdf entries flips by construction)."""
    worst = dict(cdf=0.0, samples=0.0, onehot=0.0, taps=0.0, fine=0.0)
    for M, K in PDF_MK:
        for kind in PDF_KINDS:
            c = pdf_case(kind, M, K)
            for mode in ('dense', 'lin'):
                worst['cdf'] = max(worst['cdf'], maxdiff(c[mode + '32']['cdf'], c[mode + '64']['cdf']))
                key = 'onehot' if kind == 'onehot' else 'samples'
                worst[key] = max(worst[key], maxdiff(c[mode + '32']['samples'], c[mode + '64']['samples']))
            g = rng('uniform u', kind, M, K)
            u = torch.rand(NMAX, K, generator=g)
            i32 = orc.inverse_cdf(c['bins'], c['weights'], u)[1]
            i64 = orc.inverse_cdf(c['bins'].double(), c['weights'].double(), u.double())[1]
            assert torch.equal(i32, i64), (kind, M, K)
    for S in RESAMPLE_S:
        for kind in RESAMPLE_FAMILIES:
            c = resample_case(kind, S)
            for mode in ('dense', 'lin'):
                a, b = c[mode + '32'], c[mode + '64']
                worst['taps'] = max([worst['taps']] + [maxdiff(a[k], b[k]) for k in ('weights', 'smooth', 'cdf')])
                worst['fine'] = max(worst['fine'], maxdiff(a['fine'], b['fine']))
    print('float32 vs float64 oracle: ' + ', '.join('%s %.2e' % kv for kv in worst.items()))
    assert worst['cdf'] <= W_TOL / 2 and worst['taps'] <= W_TOL / 2
    assert worst['samples'] <= MAP_TOL / 2 and worst['fine'] <= MAP_TOL / 2


def test_camera_inputs_are_well_conditioned():
    """Every camera family at every shape: the float32 oracle's raw directions within 1e-7 (half of 2e-7) of the float64
    oracle's, its unit directions within UNIT_DIR_F32 (1.49e-7, see there), origins equal after rounding; the same for the
    264 500 rays of the large raygen case; exact zeros among the direction components; rays that hit (and, over all shapes, rays that
    miss); no NaN in near / far (no parallel ray lies on a face plane: that 0 * inf is NaN in the reference too and out of
    scope).  The two fused-render scenes: float32 oracle within 5e-5 (half of 1e-4) of the float64 oracle."""
    worst, worst_unit, missed = 0.0, 0.0, False
    for kind in CAMERA_KINDS:
        zeros = False
        for H, W in CAMERA_SHAPES:
            ro, rd, un = camera_rays(kind, H, W)
            ro64, rd64, un64 = camera_rays(kind, H, W, torch.float64)
            assert torch.equal(ro, ro64.float()), (kind, H, W)
            worst, worst_unit = max(worst, maxdiff(rd, rd64)), max(worst_unit, maxdiff(un, un64))
            zeros = zeros or bool((un == 0).any())
            near, far, hit = orc.near_far(ro, un, camera_range(kind))
            assert bool(hit.any()) and bool(torch.isfinite(near).all()) and bool(torch.isfinite(far).all()), (kind, H, W)
            missed = missed or not bool(hit.all())
        assert zeros, (kind, 'no exact zero in any direction')
    ro, rd, r = hand_built_rays()
    near, far, hit = orc.near_far(ro, rd, r)
    assert bool(torch.isfinite(near).all()) and bool(torch.isfinite(far).all()) and 0 < int(hit.sum()) < hit.numel()
    print('float32 vs float64 oracle: raw directions %.2e (half bound %.1e), unit directions %.2e' % (worst, DIR_TOL / 2, worst_unit))
    assert worst <= DIR_TOL / 2 and missed
    assert worst_unit <= UNIT_DIR_F32          # see UNIT_DIR_F32: not half of 2e-7, and why
    ro, rd, un = large_raygen_rays()
    ro64, rd64, un64 = large_raygen_rays(torch.float64)
    print('large raygen case: raw directions %.2e, unit directions %.2e' % (maxdiff(rd, rd64), maxdiff(un, un64)))
    assert torch.equal(ro, ro64.float()) and maxdiff(rd, rd64) <= DIR_TOL / 2 and maxdiff(un, un64) <= UNIT_DIR_F32
    for kind in ('persp', 'ortho'):
        meta, t = render_case(kind)
        o32 = oracle_render(meta, t)
        o64 = oracle_render(meta, {k: (v.double() if v.is_floating_point() else v) for k, v in t.items()})
        d = max(maxdiff(o32[k], o64[k]) for k in ('rgb', 'depth', 'mask'))
        print('%s render, float32 vs float64 oracle: %.2e' % (kind, d))
        assert d <= ATOL / 2 and bool(o32['hit'].any()) and float(o32['mask'].mean()) > 0.05


def test_large_near_far_case_has_its_extremes_in_the_grid_stride_part():
    """The smallest near and the largest far over the hits, and some hits and misses, lie at ray indices >= 65 536; every
    hit has near >= 0.1 and far - near >= 1e-3, so the finished planes of the hits ARE the raw slab distances."""
    ro, rd, near, far, hit = large_near_far_case()
    first = 65536
    assert bool(hit[first:].any()) and not bool(hit[first:].all()) and bool(hit[:first].any()) and not bool(hit[:first].all())
    assert float(near[hit].min()) >= 0.1 and float((far - near)[hit].min()) >= 1e-3
    assert float(near[first:][hit[first:]].min()) < float(near[:first][hit[:first]].min())
    assert float(far[first:][hit[first:]].max()) > float(far[:first][hit[:first]].max())


def _composite_grad_case(na, nb, ties):
    g = rng('composite bwd', na, nb, ties)
    N = 7
    c = dict(rd=directions(N, g), t_a=depths(N, na, g),
             s_a=torch.rand(N, na, generator=g) * 8 * (torch.rand(N, na, generator=g) > 0.3),
             c_a=torch.rand(N, na, 3, generator=g) * 2 - 1, t_b=None, s_b=None, c_b=None,
             w_rgb=torch.randn(N, 3, generator=g), w_mask=torch.randn(N, generator=g))
    if nb:
        t_b = torch.rand(N, nb, generator=g) * 2 + 0.5
        if ties:
            t_b[:, 0::2] = c['t_a'][:, torch.randint(0, na, (len(range(0, nb, 2)),), generator=g)]
            t_b[:, -1] = t_b[:, 0]
        c.update(t_b=t_b, s_b=torch.rand(N, nb, generator=g) * 20, c_b=torch.rand(N, nb, 3, generator=g) * 2 - 1)
    return c


COMPOSITE_BWD = [(2, 0, False), (129, 0, False), (257, 0, False), (512, 0, False), (128, 1, False), (1, 128, False),
                 (64, 65, False), (64, 65, True), (64, 64, True)]


@functools.lru_cache(maxsize=None)
def composite_grads(na, nb, ties, white, dt):
    c = _composite_grad_case(na, nb, ties)
    names = ['rd', 's_a', 'c_a'] + (['s_b', 'c_b'] if nb else [])
    leaf = {k: c[k].to(dt).requires_grad_() for k in names}
    rgb, acc, _ = oracle_merge_composite(leaf['rd'], c['t_a'].to(dt), leaf['s_a'], leaf['c_a'],
                                         c['t_b'].to(dt) if nb else None, leaf.get('s_b'), leaf.get('c_b'), None, None, white)
    loss = (rgb * c['w_rgb'].to(dt)).sum() + (acc * c['w_mask'].to(dt)).sum()
    return dict(zip(names, torch.autograd.grad(loss, [leaf[k] for k in names])))


def rel_err(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-12))


def test_composite_backward_inputs_are_well_conditioned():
    """float32 autograd of the oracle within 1e-4 (half of rel_close's 2e-4) of its float64 autograd, every case."""
    worst = 0.0
    for na, nb, ties in COMPOSITE_BWD:
        for white in (True, False):
            g32, g64 = (composite_grads(na, nb, ties, white, dt) for dt in (torch.float32, torch.float64))
            worst = max([worst] + [rel_err(g32[k], g64[k]) for k in g64])
    print('float32 vs float64 oracle gradients: %.2e (half bound %.1e)' % (worst, GRAD_TOL / 2))
    assert worst <= GRAD_TOL / 2


POINTS_BWD = [(S, N) for S in (1, 63, 65, 512) for N in (7, 2)]
RAYGEN_BWD_SHAPE = (3, 19, 23)


@functools.lru_cache(maxsize=None)
def points_bwd_case(S, N):
    g = rng('points bwd', S, N)
    return dict(ro=torch.randn(N, 3, generator=g), rd=torch.randn(N, 3, generator=g), t=torch.rand(N, S, generator=g) + 0.5,
                w=torch.randn(N, S, 3, generator=g))


@functools.lru_cache(maxsize=None)
def points_bwd_grads(S, N, dt):
    c = points_bwd_case(S, N)
    a, b = c['ro'].to(dt).requires_grad_(), c['rd'].to(dt).requires_grad_()
    return torch.autograd.grad((orc.points_on_rays(a, b, c['t'].to(dt)) * c['w'].to(dt)).sum(), (a, b))


@functools.lru_cache(maxsize=None)
def raygen_bwd_case(with_bbox):
    g = rng('raygen bwd', with_bbox)
    B, H, W = RAYGEN_BWD_SHAPE
    cam = torch.zeros(B, 4, 4)
    cam[:, :3, :3] = torch.linalg.qr(torch.randn(B, 3, 3, generator=g))[0]
    cam[:, :3, 3] = torch.randn(B, 3, generator=g)
    cam[:, 3, 3] = 1.0
    return dict(cam2world=cam, focal=torch.rand(B, generator=g) + 0.8, center=torch.rand(B, 2, generator=g) * 0.5 + 0.25,
                bbox=torch.stack((torch.rand(B, 2, generator=g) - 1.0, torch.rand(B, 2, generator=g) + 1.0), dim=1)
                if with_bbox else None,
                w_o=torch.randn(B, H, W, 3, generator=g), w_d=torch.randn(B, H, W, 3, generator=g))


@functools.lru_cache(maxsize=None)
def raygen_bwd_grads(with_bbox, normalize, dt):
    """(g_cam2world [B,4,4], g_focal [B]): autograd of orc.ray_bundle (+ unit_dirs) in `dt`"""
    B, H, W = RAYGEN_BWD_SHAPE
    c = to_(raygen_bwd_case(with_bbox), dt)
    cam, focal = c['cam2world'].clone().requires_grad_(), c['focal'].clone().requires_grad_()
    ro, rd = orc.ray_bundle(H, W, focal, cam, c['bbox'], c['center'])
    if normalize:
        rd = orc.unit_dirs(rd)
    return torch.autograd.grad((ro * c['w_o']).sum() + (rd * c['w_d']).sum(), (cam, focal))


def test_ray_backward_inputs_are_well_conditioned():
    """float32 autograd of the oracle within 1e-4 (half of rel_close's 2e-4) of its float64 autograd for every case of the
    points-backward and raygen-backward tests (the whole cam2world gradient on its own scale, and the focal gradient)."""
    worst = 0.0
    for S, N in POINTS_BWD:
        g32, g64 = points_bwd_grads(S, N, torch.float32), points_bwd_grads(S, N, torch.float64)
        worst = max([worst] + [rel_err(a, b) for a, b in zip(g32, g64)])
    for with_bbox in (False, True):
        for normalize in (True, False):
            g32, g64 = (raygen_bwd_grads(with_bbox, normalize, dt) for dt in (torch.float32, torch.float64))
            worst = max([worst] + [rel_err(a, b) for a, b in zip(g32, g64)])
    print('float32 vs float64 oracle gradients (points, raygen): %.2e (half bound %.1e)' % (worst, GRAD_TOL / 2))
    assert worst <= GRAD_TOL / 2


# ------------------------------------------------------------------------------------------------
# on the GPU: helpers
# ------------------------------------------------------------------------------------------------
def sentinel(dtype):
    return 171 if dtype == torch.uint8 else -777


def out_buf(dev, n, *tail, dtype=torch.float32):
    """[n + GUARD, *tail] filled with the sentinel: rows [0,n) are the kernel's, the rest must come back untouched"""
    return torch.full((n + GUARD, *tail), sentinel(dtype), dtype=dtype, device=dev)


def take(buf, n, what):
    assert bool((buf[n:] == sentinel(buf.dtype)).all()), '%s: rows behind the last of %d rays were written' % (what, n)
    got = buf[:n].cpu()
    assert not bool((got == sentinel(buf.dtype)).all()) or n == 0, '%s: nothing was written' % what
    return got


def launch(dev, fname, sname, **kw):
    with torch.cuda.device(dev):
        _lib.call_struct(fname, sname, torch.cuda.current_stream(dev).cuda_stream, **kw)


def dev_(c, dev, keys):
    return {k: (None if c[k] is None else c[k].contiguous().to(dev)) for k in keys}


# ------------------------------------------------------------------------------------------------
# 2. forward stages
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('S', WEIGHT_S)
def test_ray_weights(gpu_device, S):
    """ray_weights_kernel<2> up to S = 128 and <8> from 129 (both sides of the switch; 63 / 64 / 65: the slot boundary of
    the scan, 511 / 512: the last lane of the last slot), every sigma family, non-unit directions; N = 1, 2, 3, 5, 9: one to
    three idle waves behind the last ray, which must write nothing."""
    dev = gpu_device
    for kind in FAMILIES:
        c = weights_case(kind, S)
        d = dev_(c, dev, ('sigma', 'rd', 't'))
        for N in NS:
            w = out_buf(dev, N, S)
            launch(dev, 'nfi_ray_weights', 'nfi_weights_args', n_rays=N, n_samples=S, sigma=d['sigma'], ray_directions=d['rd'],
                   depth=d['t'], weights=w)
            close(take(w, N, 'weights'), c['w64'][:N], W_TOL, 'weights %s S=%d N=%d' % (kind, S, N))


@pytest.mark.gpu
@pytest.mark.parametrize('M,K', PDF_MK)
def test_sample_pdf(gpu_device, M, K):
    """sample_pdf_kernel with M and K independent of each other: pivot tables of 1 (M <= 8) to 16 (M = 128) live entries
    (8 / 9, 63 / 64 / 65, 127 / 128: both sides of a pivot and of the slot boundary), K on both sides of the 64-lane slot,
    u dense and as one broadcast row (u_row_stride = 0), u = 0, u on the row's own cdf entries, u = 1 - 2^-24 and u = 1.0
    (>= the last cdf entry: all pivots counted, index M), all-zero / one-hot rows (the `den < 1e-5` switch), idle waves
    behind N = 1, 2, 3, 5, 9 rays.  cdf against float64 (1e-6); indices bit-exact against searchsorted on the kernel's own
    cdf; samples against the oracle's interpolation on that cdf (1e-5) and - all but the one-hot rows, which sit on the
    reference's switch (see the conditioning test) - against the float64 oracle (1e-5); with inds and cdf NULL the samples
    are the same bits."""
    dev = gpu_device
    for kind in PDF_KINDS:
        c = pdf_case(kind, M, K)
        d = dev_(c, dev, ('bins', 'weights', 'dense', 'lin'))
        for mode, stride in (('dense', K), ('lin', 0)):
            ref, u_cpu = c[mode + '64'], (c['dense'] if mode == 'dense' else c['lin'].expand(NMAX, K))
            for N in NS:
                what = '%s %s M=%d K=%d N=%d' % (kind, mode, M, K, N)
                smp, inds, cdf = out_buf(dev, N, K), out_buf(dev, N, K, dtype=torch.int64), out_buf(dev, N, M)
                args = dict(n_rays=N, n_bins=M, n_samples=K, bins=d['bins'], weights=d['weights'], u=d[mode], u_row_stride=stride)
                launch(dev, 'nfi_sample_pdf', 'nfi_sample_pdf_args', samples=smp, inds=inds, cdf=cdf, **args)
                smp, inds, cdf = take(smp, N, 'samples'), take(inds, N, 'inds'), take(cdf, N, 'cdf')
                close(cdf, ref['cdf'][:N], W_TOL, 'cdf ' + what)
                own, own_inds = interpolate_on_cdf(c['bins'][:N], cdf, u_cpu[:N])
                exact(inds, own_inds, 'indices on the own cdf ' + what)
                close(smp, own, MAP_TOL, 'samples on the own cdf ' + what)
                if kind != 'onehot':
                    close(smp, ref['samples'][:N], MAP_TOL, 'samples ' + what)
                bare = out_buf(dev, N, K)
                launch(dev, 'nfi_sample_pdf', 'nfi_sample_pdf_args', samples=bare, inds=None, cdf=None, **args)
                exact(take(bare, N, 'samples'), smp, 'samples without inds / cdf ' + what)


@pytest.mark.gpu
@pytest.mark.parametrize('S', RESAMPLE_S)
def test_resample(gpu_device, S):
    """resample_kernel up to S = 64 (M = 63 bins: 8 pivots, the last one +inf) and resample_wide_kernel from 65 (M = 64: the
    pivot table grows to 16); 65 and 66: the lane-63 -> lane-0 hand-over of smooth_weights_wide and next_elem between the two
    slots; 4 / 5 / 8 / 9: fewer bins than one pivot block; all taps, dense and broadcast u, idle waves behind N = 1 .. 9."""
    dev = gpu_device
    for kind in RESAMPLE_FAMILIES:
        c = resample_case(kind, S)
        d = dev_(c, dev, ('sigma', 'rd', 't', 'dense', 'lin'))
        for mode, stride in (('dense', S), ('lin', 0)):
            ref, u_cpu = c[mode + '64'], (c['dense'] if mode == 'dense' else c['lin'].expand(NMAX, S))
            for N in NS:
                what = '%s %s S=%d N=%d' % (kind, mode, S, N)
                o = dict(fine_depth=out_buf(dev, N, S), weights=out_buf(dev, N, S), smooth=out_buf(dev, N, S),
                         cdf=out_buf(dev, N, S - 1), inds=out_buf(dev, N, S, dtype=torch.int64))
                args = dict(n_rays=N, n_samples=S, sigma=d['sigma'], ray_directions=d['rd'], depth=d['t'], u=d[mode],
                            u_row_stride=stride)
                launch(dev, 'nfi_resample', 'nfi_resample_args', **args, **o)
                o = {k: take(v, N, k) for k, v in o.items()}
                close(o['weights'], ref['weights'][:N], W_TOL, 'weights ' + what)
                close(o['smooth'], ref['smooth'][:N], W_TOL, 'smoothed weights ' + what)
                close(o['cdf'], ref['cdf'][:N], W_TOL, 'cdf ' + what)
                exact(o['inds'], torch.searchsorted(o['cdf'].contiguous(), u_cpu[:N].contiguous(), right=True),
                      'indices on the own cdf ' + what)
                close(o['fine_depth'], ref['fine'][:N], MAP_TOL, 'fine depths ' + what)
                bare = out_buf(dev, N, S)
                launch(dev, 'nfi_resample', 'nfi_resample_args', fine_depth=bare, **args)
                exact(take(bare, N, 'fine'), o['fine_depth'], 'fine depths without taps ' + what)


@pytest.mark.gpu
@pytest.mark.parametrize('na,nb', COMPOSITE_LISTS)
def test_composite_forward(gpu_device, na, nb):
    """composite_kernel<2> (n_a + n_b <= 128), <4> (<= 256), <8>: 128 / 129 and 256 / 257 samples, as one list and as two
    lists of unequal lengths (merge_scatter's general ranking; list b of one sample, list a of one sample); the tie path of
    the ranking - b equal to an entry of a, two equal entries of b, all depths equal - where perm and depth_sorted must be
    torch.sort(cat(a, b), stable=True) on every ray; both backgrounds; 0, 1, 14, 33 extra channels; idle waves behind
    N = 1 .. 9 rays."""
    dev = gpu_device
    c = composite_case(na, nb)
    d = dev_(c, dev, ('rd', 't_a', 's_a', 'c_a', 't_b', 's_b', 'c_b'))
    n = na + nb
    for n_extra in EXTRAS:
        e_a = c['e_a'][..., :n_extra].contiguous().to(dev) if n_extra else None
        e_b = c['e_b'][..., :n_extra].contiguous().to(dev) if n_extra and nb else None
        for white in (True, False):
            ref = composite_ref(na, nb, white, n_extra, torch.float64)
            for N in NS:
                what = 'n_a=%d n_b=%d extra=%d white=%d N=%d' % (na, nb, n_extra, white, N)
                o = dict(rgb_map=out_buf(dev, N, 3), depth_map=out_buf(dev, N), mask=out_buf(dev, N),
                         extra_map=out_buf(dev, N, n_extra) if n_extra else None, weights=out_buf(dev, N, n),
                         depth_sorted=out_buf(dev, N, n), perm=out_buf(dev, N, n, dtype=torch.int64))
                launch(dev, 'nfi_composite_fwd', 'nfi_composite_args', n_rays=N, n_a=na, n_b=nb, ray_directions=d['rd'],
                       depth_a=d['t_a'], sigma_a=d['s_a'], rgb_a=d['c_a'], depth_b=d['t_b'], sigma_b=d['s_b'], rgb_b=d['c_b'],
                       n_extra=n_extra, extra_a=e_a, extra_b=e_b, white_background=int(white), **o)
                o = {k: take(v, N, k) for k, v in o.items() if v is not None}
                exact(o['perm'], ref['perm'][:N], 'permutation ' + what)
                exact(o['depth_sorted'], ref['depth_sorted'][:N], 'sorted depths ' + what)
                close(o['weights'], ref['weights'][:N], W_TOL, 'weights ' + what)
                close(o['rgb_map'], ref['rgb'][:N], MAP_TOL, 'rgb map ' + what)
                close(o['depth_map'], ref['depth'][:N], MAP_TOL, 'depth map ' + what)
                close(o['mask'], ref['mask'][:N], MAP_TOL, 'mask ' + what)
                if n_extra:
                    close(o['extra_map'], ref['extra'][:N], MAP_TOL, 'extra map ' + what)


@pytest.mark.gpu
@pytest.mark.parametrize('S', STRATIFIED_S)
def test_stratified_points_and_points_on_rays(gpu_device, S):
    """stratified_kernel / points_on_rays_kernel (one thread per sample): N * S below, at and beyond one block of 256 and
    no multiple of it, with and without noise, near == far on two rays (lerp of a zero-length interval, noise times zero);
    the threads behind the last sample write nothing.  Bit-exact against the float32 oracle."""
    dev = gpu_device
    g = rng('stratified', S)
    ro, rd = torch.randn(NMAX, 3, generator=g), directions(NMAX, g)
    near = torch.rand(NMAX, generator=g) + 0.3
    far = near + torch.rand(NMAX, generator=g) * 2
    far[1], far[4] = near[1], near[4]
    noise = torch.rand(NMAX, S, generator=g)
    d = {k: v.to(dev) for k, v in dict(ro=ro, rd=rd, near=near, far=far, noise=noise).items()}
    for jitter in (True, False):
        t_ref = orc.stratified_depths(near, far, S, noise if jitter else None)
        x_ref = orc.points_on_rays(ro, rd, t_ref)
        t_dev = t_ref.contiguous().to(dev)
        for N in NS:
            what = 'S=%d noise=%d N=%d' % (S, jitter, N)
            dep, pts = out_buf(dev, N, S), out_buf(dev, N, S, 3)
            launch(dev, 'nfi_stratified_points', 'nfi_stratified_args', n_rays=N, n_samples=S, ray_origins=d['ro'],
                   ray_directions=d['rd'], near_plane=d['near'], far_plane=d['far'], noise=d['noise'] if jitter else None,
                   depth=dep, points=pts)
            exact(take(dep, N, 'depths'), t_ref[:N], 'stratified depths ' + what)
            exact(take(pts, N, 'points'), x_ref[:N], 'query points ' + what)
            pts = out_buf(dev, N, S, 3)
            with torch.cuda.device(dev):
                _lib.check(_lib.load().nfi_points_on_rays(_lib.ptr(d['ro']), _lib.ptr(d['rd']), _lib.ptr(t_dev), N, S, _lib.ptr(pts),
                                                          torch.cuda.current_stream(dev).cuda_stream), 'nfi_points_on_rays')
            exact(take(pts, N, 'points'), x_ref[:N], 'points_on_rays ' + what)


# ------------------------------------------------------------------------------------------------
# 3. rays and the cube
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('kind', CAMERA_KINDS)
def test_axis_aligned_cameras(gpu_device, kind):
    """make_ray and slab_test with exact 0 and -0 in rotations and directions (1 / d = +-inf, the hand-written NaN / inf
    semantics of ATen's min / max): identity pose, the six axis views, orthographic views with cam2world[3,3] != 1, with
    bbox and principal point, at 1 x N, N x 1, even and odd widths.  Origins exact, directions 2e-7 of the float32 oracle (the suite's reference
    for that bound; its distance from float64 is in the conditioning test); near, far and hit of
    ops.near_far on the oracle's own rays exact.  (Parallel rays with the origin ON a face plane are 0 * inf = NaN in the
    reference as well: out of scope, no input here has one.)"""
    dev = gpu_device
    c = to_(camera(kind), dev=dev)
    for H, W in CAMERA_SHAPES:
        what = '%s %dx%d' % (kind, H, W)
        ro, rd, un = camera_rays(kind, H, W)
        h_ro, h_rd = ops.raygen(H, W, c['focal'], c['cam2world'], c['bbox'], c['center'], normalize=False)
        exact(h_ro, ro, 'origins ' + what)
        close(h_rd, rd, DIR_TOL, 'raw directions ' + what)
        h_ro, h_un = ops.raygen(H, W, c['focal'], c['cam2world'], c['bbox'], c['center'], normalize=True)
        exact(h_ro, ro, 'origins ' + what)
        close(h_un, un, DIR_TOL, 'unit directions ' + what)
        near, far, hit = orc.near_far(ro, un, camera_range(kind))
        h_near, h_far, h_hit = ops.near_far(ro.to(dev), un.contiguous().to(dev), camera_range(kind))
        exact(h_near, near, 'near ' + what); exact(h_far, far, 'far ' + what); exact(h_hit, hit, 'hit ' + what)


@pytest.mark.gpu
def test_hand_built_rays_with_zero_components(gpu_device):
    """slab_test on rays whose directions hold exact 0 and -0: through the cube along an axis, from inside it (near < 0 ->
    the 0.1 clamp of finish_planes), parallel beside it (lo = hi = -inf decide the miss), grazing an edge (far - near < 1e-3
    -> far = near + 1e-3); then one ray that hits among misses (the batch-wide fill comes from that one ray).  10 and 5
    rays: idle lanes and waves of slab_kernel's only block.  Exact against the oracle.  (No parallel ray starts on a face
    plane: 0 * inf is NaN in the reference too.)"""
    dev = gpu_device
    ro, rd, r = hand_built_rays()
    for pick in (slice(None), [5, 3, 8, 0, 5]):
        o, d = ro[pick].contiguous(), rd[pick].contiguous()
        near, far, hit = orc.near_far(o, d, r)
        h_near, h_far, h_hit = ops.near_far(o.to(dev), d.to(dev), r)
        exact(h_near, near, 'near'); exact(h_far, far, 'far'); exact(h_hit, hit, 'hit')
    assert int(hit.sum()) == 1


@pytest.mark.gpu
def test_raygen_grid_stride_pass(gpu_device):
    """raygen_kernel's grid is capped at 1024 blocks: 5 x 230 x 230 = 264 500 rays are 2 356 more than its 262 144 threads,
    so the last rows of the fifth image come from the second trip of the grid-stride loop (another scene index, with a
    principal point).  Origins exact, raw and unit directions 2e-7 of the float32 oracle, every ray."""
    dev = gpu_device
    B, H, W = LARGE_RAYGEN
    c = large_raygen_case()
    ro, rd, un = large_raygen_rays()
    d = to_(c, dev=dev)
    for normalize in (False, True):
        ro_buf, rd_buf = out_buf(dev, B * H * W, 3), out_buf(dev, B * H * W, 3)
        launch(dev, 'nfi_raygen', 'nfi_raygen_args', n_scenes=B, height=H, width=W, cam2world=d['cam2world'], focal=d['focal'],
               bbox=None, center=d['center'], normalize=int(normalize), ray_origins=ro_buf, ray_directions=rd_buf)
        exact(take(ro_buf, B * H * W, 'origins').view(B, H, W, 3), ro, 'origins')
        close(take(rd_buf, B * H * W, 'directions').view(B, H, W, 3), un if normalize else rd, DIR_TOL,
              'directions normalize=%d' % normalize)


@pytest.mark.gpu
def test_near_far_grid_stride_pass(gpu_device):
    """slab_kernel's grid is capped at 256 blocks: of 70 001 rays the last 4 465 come from the second trip of the grid-stride
    loop, and the smallest near, the largest far and part of the hit count - what the atomicMax / atomicAdd into the three
    reduce cells must deliver - exist only there (the CPU test above asserts that of the input).  near, far, hit of every
    ray and the four reduce cells exact against the oracle; the raw distances of the hits equal their finished planes."""
    dev = gpu_device
    n = LARGE_NEAR_FAR
    ro, rd, near, far, hit = large_near_far_case()
    o = dict(near_raw=out_buf(dev, n), far_raw=out_buf(dev, n), hit=out_buf(dev, n, dtype=torch.uint8),
             reduce=torch.full((4 + GUARD,), -777, dtype=torch.int32, device=dev), near_plane=out_buf(dev, n),
             far_plane=out_buf(dev, n))
    ro_dev, rd_dev = ro.to(dev), rd.to(dev)
    launch(dev, 'nfi_near_far', 'nfi_near_far_args', n_rays=n, ray_origins=ro_dev, ray_directions=rd_dev, scene_range=0.5, **o)
    red = o.pop('reduce').cpu()
    o = {k: take(v, n, k) for k, v in o.items()}
    exact((o['hit'] & 1).bool(), hit, 'hit')
    exact(o['near_plane'], near, 'near'); exact(o['far_plane'], far, 'far')
    exact(o['near_raw'][hit], near[hit], 'raw near of the hits'); exact(o['far_raw'][hit], far[hit], 'raw far of the hits')
    assert bool((red[4:] == -777).all()), 'reduce: written behind its four cells'
    cells = [int(v) & 0xFFFFFFFF for v in red[:4]]
    want = [~ordered_key(near[hit].min()) & 0xFFFFFFFF, ordered_key(far[hit].max()), int(hit.sum()), 0]
    assert cells == want, (cells, want)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['persp', 'ortho'])
def test_fused_render_under_axis_aligned_cameras(gpu_device, kind):
    """The render set-up kernel shares make_ray and slab_test with the stage kernels: one fused render (2 x 6 x 8 pixels,
    S = 16, fine pass) from the perspective identity pose (inside the cube) and from axis-aligned orthographic cameras with
    cam2world[3,3] = 1.25 (every direction has two exact zeros), with and without skipping missed rays, against orc.render
    at the suite's 1e-4."""
    meta, t = render_case(kind)
    ref = oracle_render(meta, t)
    for skip in (False, True):
        out = hip_render(meta, t, gpu_device, skip_missed_rays=skip)
        for k in ('rgb', 'depth', 'mask'):
            close(out[k], ref[k], ATOL, '%s %s skip=%d' % (kind, k, skip))


# ------------------------------------------------------------------------------------------------
# 4. backward
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('na,nb,ties', COMPOSITE_BWD)
def test_composite_backward_at_the_switches(gpu_device, na, nb, ties):
    """composite_bwd_kernel<2> / <4> / <8> on both sides of 128 / 129 and 256 / 257 samples, as one list (2, 129, 257, 512)
    and as two lists of unequal lengths (128 + 1, 1 + 128, 64 + 65: merge_scatter's general ranking), dense and in the stash
    layout (list_row_stride = n_a + n_b, list b inside list a's rows), and with tied depths - through the general ranking
    (64 + 65) and through merge_pair_scatter (64 + 64) - where the forward's stable order decides which of two samples at
    one depth gets which gradient.  7 rays: one idle wave.  Against float64 autograd of the oracle, rel_close."""
    dev = gpu_device
    c = _composite_grad_case(na, nb, ties)
    d = dev_(c, dev, ('rd', 't_a', 's_a', 'c_a', 't_b', 's_b', 'c_b', 'w_rgb', 'w_mask'))
    N, n = c['rd'].shape[0], na + nb
    for white in (True, False):
        ref = composite_grads(na, nb, ties, white, torch.float64)
        got = ops.composite_bwd(d['rd'], d['t_a'], d['s_a'], d['c_a'], d['w_rgb'], d['w_mask'], d['t_b'], d['s_b'], d['c_b'],
                                white_background=white)
        pairs = [('rd', 'g_ray_directions'), ('s_a', 'g_sigma_a'), ('c_a', 'g_rgb_a')] + \
                ([('s_b', 'g_sigma_b'), ('c_b', 'g_rgb_b')] if nb else [])
        for r, k in pairs:
            rel_close(got[k], ref[r], 'dense %s n_a=%d n_b=%d ties=%d white=%d' % (k, na, nb, ties, white))
        # the stash layout: rows of n_a + n_b entries, list a in front, list b behind it
        row = lambda a, b: torch.cat((a, b), dim=1).contiguous() if nb else a.contiguous()
        t, s, col = row(d['t_a'], d['t_b']), row(d['s_a'], d['s_b']), row(d['c_a'], d['c_b'])
        g_s, g_c, g_rd = out_buf(dev, N, n), out_buf(dev, N, n, 3), out_buf(dev, N, 3)
        off = lambda x, per: x.data_ptr() + 4 * per * na
        launch(dev, 'nfi_composite_bwd', 'nfi_composite_bwd_args', n_rays=N, n_a=na, n_b=nb, list_row_stride=n,
               ray_directions=d['rd'], depth_a=t, sigma_a=s, rgb_a=col, depth_b=off(t, 1) if nb else None,
               sigma_b=off(s, 1) if nb else None, rgb_b=off(col, 3) if nb else None, n_extra=0, white_background=int(white),
               g_rgb_map=d['w_rgb'], g_mask=d['w_mask'], g_sigma_a=g_s, g_rgb_a=g_c, g_sigma_b=off(g_s, 1) if nb else None,
               g_rgb_b=off(g_c, 3) if nb else None, g_ray_directions=g_rd)
        g_s, g_c, g_rd = take(g_s, N, 'g_sigma'), take(g_c, N, 'g_rgb'), take(g_rd, N, 'g_rd')
        what = 'stash n_a=%d n_b=%d ties=%d white=%d' % (na, nb, ties, white)
        rel_close(g_rd, ref['rd'], 'g_rd ' + what)
        rel_close(g_s[:, :na], ref['s_a'], 'g_sigma_a ' + what); rel_close(g_c[:, :na], ref['c_a'], 'g_rgb_a ' + what)
        if nb:
            rel_close(g_s[:, na:], ref['s_b'], 'g_sigma_b ' + what); rel_close(g_c[:, na:], ref['c_b'], 'g_rgb_b ' + what)


@pytest.mark.gpu
@pytest.mark.parametrize('S', sorted({S for S, _ in POINTS_BWD}))
def test_points_backward_sizes(gpu_device, S):
    """points_bwd_kernel (one wave per ray, lanes stride over the samples): S = 1 (63 lanes add nothing), 63 / 65 (the
    second trip of the lane loop starts at 65), 512 (eight trips); 7 and 2 rays: idle waves, which must write nothing."""
    dev = gpu_device
    for N in (7, 2):
        c = points_bwd_case(S, N)
        t, w = c['t'], c['w']
        ref = points_bwd_grads(S, N, torch.float64)
        g_ro, g_rd = out_buf(dev, N, 3), out_buf(dev, N, 3)
        w_dev, t_dev = w.to(dev), t.to(dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().nfi_points_bwd(_lib.ptr(w_dev), _lib.ptr(t_dev), N, S, _lib.ptr(g_ro), _lib.ptr(g_rd),
                                                  torch.cuda.current_stream(dev).cuda_stream), 'nfi_points_bwd')
        rel_close(take(g_ro, N, 'g_ro'), ref[0], 'g_ro S=%d N=%d' % (S, N))
        rel_close(take(g_rd, N, 'g_rd'), ref[1], 'g_rd S=%d N=%d' % (S, N))


@pytest.mark.gpu
@pytest.mark.parametrize('ordered', [False, True])
@pytest.mark.parametrize('with_bbox', [False, True])
def test_raygen_backward_with_principal_point(gpu_device, with_bbox, ordered):
    """raygen_bwd_pixel's `center` branch (u - 0.5 (2c - 1) - 0.5), without and with a bbox behind it, in raygen_bwd_kernel
    (two blocks per image, atomics) and raygen_bwd_ordered_kernel (one block per image, two trips of its pixel loop), at a
    non-square 19 x 23 image, normalised and raw directions.  Against float64 autograd of orc.ray_bundle, rel_close."""
    dev = gpu_device
    B, H, W = RAYGEN_BWD_SHAPE
    c = to_(raygen_bwd_case(with_bbox), dev=dev)
    for normalize in (True, False):
        ref_cam, ref_focal = raygen_bwd_grads(with_bbox, normalize, torch.float64)
        g_cam, g_focal = ops.raygen_bwd(H, W, c['focal'], c['cam2world'], c['bbox'], c['center'], normalize, c['w_o'], c['w_d'],
                                        ordered=ordered)
        what = 'bbox=%d ordered=%d normalize=%d' % (with_bbox, ordered, normalize)
        rel_close(g_cam, ref_cam, 'g_cam2world (all sixteen entries; the bottom row is 0 for a perspective camera) ' + what)
        rel_close(g_focal, ref_focal, 'g_focal ' + what)


# ------------------------------------------------------------------------------------------------
# 5. wrappers refuse malformed arguments before they launch
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_wrappers_refuse_mismatched_shapes(gpu_device):
    """No kernel runs here: ops.sample_pdf, resample, ray_weights, composite and composite_bwd raise ValueError on arguments
    whose row counts or last dimensions disagree (the kernels index by the shape of depth / bins alone and would read past
    the shorter buffer), and accept the broadcast u row (stride 0) whatever the number of rays."""
    dev = gpu_device
    z = lambda *s: torch.zeros(*s, device=dev)
    n, M, K, S = 6, 9, 5, 8
    bad = {
        'sample_pdf: u with fewer rows': lambda: ops.sample_pdf(z(n, M), z(n, M - 1), z(n - 1, K)),
        'sample_pdf: weights [n, M]': lambda: ops.sample_pdf(z(n, M), z(n, M), z(n, K)),
        'sample_pdf: weights with fewer rows': lambda: ops.sample_pdf(z(n, M), z(n - 1, M - 1), z(n, K)),
        'sample_pdf: one dense u row for n rays': lambda: ops.sample_pdf(z(n, M), z(n, M - 1), z(1, K)),
        'resample: u with fewer rows': lambda: ops.resample(z(n, S), z(n, 3), z(n, S), z(n - 1, S)),
        'resample: u of another length': lambda: ops.resample(z(n, S), z(n, 3), z(n, S), z(n, S - 1)),
        'resample: sigma vs depth': lambda: ops.resample(z(n, S - 1), z(n, 3), z(n, S), z(n, S)),
        'resample: directions vs depth': lambda: ops.resample(z(n, S), z(n - 1, 3), z(n, S), z(n, S)),
        'ray_weights: sigma vs depth': lambda: ops.ray_weights(z(n, S + 1), z(n, 3), z(n, S)),
        'ray_weights: sigma rows': lambda: ops.ray_weights(z(n - 1, S), z(n, 3), z(n, S)),
        'ray_weights: directions': lambda: ops.ray_weights(z(n, S), z(n + 1, 3), z(n, S)),
        'composite: sigma vs depth': lambda: ops.composite(z(n, 3), z(n, S), z(n, S - 1), z(n, S, 3)),
        'composite: rgb vs depth': lambda: ops.composite(z(n, 3), z(n, S), z(n, S), z(n - 1, S, 3)),
        'composite: directions': lambda: ops.composite(z(n - 1, 3), z(n, S), z(n, S), z(n, S, 3)),
        'composite: list b rows': lambda: ops.composite(z(n, 3), z(n, S), z(n, S), z(n, S, 3), z(n - 1, 4), z(n - 1, 4), z(n - 1, 4, 3)),
        'composite: sigma_b vs depth_b': lambda: ops.composite(z(n, 3), z(n, S), z(n, S), z(n, S, 3), z(n, 4), z(n, 5), z(n, 4, 3)),
        'composite: extra vs depth': lambda: ops.composite(z(n, 3), z(n, S), z(n, S), z(n, S, 3), extra_a=z(n, S - 1, 2)),
        'composite: extra_b missing': lambda: ops.composite(z(n, 3), z(n, S), z(n, S), z(n, S, 3), z(n, 4), z(n, 4), z(n, 4, 3),
                                                            extra_a=z(n, S, 2)),
        'composite: extra_b channels': lambda: ops.composite(z(n, 3), z(n, S), z(n, S), z(n, S, 3), z(n, 4), z(n, 4), z(n, 4, 3),
                                                             extra_a=z(n, S, 2), extra_b=z(n, 4, 3)),
        'composite_bwd: sigma vs depth': lambda: ops.composite_bwd(z(n, 3), z(n, S), z(n, S - 1), z(n, S, 3), z(n, 3)),
        'composite_bwd: g_rgb_map rows': lambda: ops.composite_bwd(z(n, 3), z(n, S), z(n, S), z(n, S, 3), z(n - 1, 3)),
        'composite_bwd: g_mask rows': lambda: ops.composite_bwd(z(n, 3), z(n, S), z(n, S), z(n, S, 3), z(n, 3), z(n - 1)),
        'composite_bwd: list b rows': lambda: ops.composite_bwd(z(n, 3), z(n, S), z(n, S), z(n, S, 3), z(n, 3), None, z(n - 1, 4),
                                                                z(n - 1, 4), z(n - 1, 4, 3)),
        'composite_bwd: extra_b missing': lambda: ops.composite_bwd(z(n, 3), z(n, S), z(n, S), z(n, S, 3), z(n, 3), None, z(n, 4),
                                                                    z(n, 4), z(n, 4, 3), extra_a=z(n, S, 2), g_extra_map=z(n, 2)),
        'composite_bwd: g_extra_map': lambda: ops.composite_bwd(z(n, 3), z(n, S), z(n, S), z(n, S, 3), z(n, 3), None,
                                                                extra_a=z(n, S, 2), g_extra_map=z(n, 3)),
    }
    for what, call in bad.items():
        # the message must be the new check's own ('<wrapper>: ...'), not an incidental error from further inside
        with pytest.raises(ValueError, match='^' + re.escape(what.split(':')[0] + ':')):
            call()
    # what must still pass: one broadcast row for any number of rays
    smp, _, _ = ops.sample_pdf(torch.linspace(0.5, 1.5, M, device=dev).repeat(n, 1), torch.ones(n, M - 1, device=dev),
                               torch.linspace(0, 1, K, device=dev).expand(n, K))
    assert tuple(smp.shape) == (n, K) and bool(torch.isfinite(smp).all())
