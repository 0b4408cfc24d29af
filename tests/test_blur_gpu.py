"""filters.blur / filters.filt2d / ops.separable_filter (csrc/nfi_filter.inc, separable_filter_kernel) on the GPU against the
float64 restatement of lib/ops.py:29-55 (tests/blur_util.py, pinned to the live reference by tests/test_blur_abi.py).

Sizes: 1 x 1, 5 x 9 and 16 x 16 (smaller than the largest radius), 37 x 53, 128 x 128 (4 x 4 tiles), and around the kernel's
tile of 32 x 32 outputs: 31 x 33, 32 x 32, 33 x 31.  B in {1, 3} and C in {1, 3, 4}, two pairs per size, every pair twice or
more over the list; every case in both input layouts, at i = 0, 6250, 11000, 12083 (r = 30, 15, 3, 1), on both backgrounds.

The parity bound is min(2 x e32 + 2^-21, 2e-5) per element.  e32 is computed here, never by the code under test: the worst
distance of the reference's own ops.blur - PyTorch-ROCm on this GPU, the same inputs - to the float64 restatement over all
parity cases of this file.  The factor 2 is for another summation order, 2^-21 is four units in the last place of 1.0 for
cases where the reference is exact, and the cap keeps a loose library convolution from hiding a failure (a dropped outermost
tap at r = 30 costs about 9e-5)."""
import functools
import os
import re

import pytest
import torch

from nerf_from_image_amd import _lib
from oracle import reference
import blur_util as bu

TILE_H, TILE_W = 32, 32           # kFilterTileH, kFilterTileW of csrc/nfi_filter.inc (test_tile_constants holds them to it)
SHAPES = [(B, C, H, W) for (H, W), pairs in (
    ((1, 1), ((1, 1), (3, 4))),
    ((5, 9), ((1, 3), (3, 1))),
    ((16, 16), ((3, 4), (1, 1))),
    ((37, 53), ((1, 4), (3, 3))),
    ((128, 128), ((3, 4), (1, 3))),
    ((TILE_H - 1, TILE_W + 1), ((3, 1), (1, 4))),
    ((TILE_H, TILE_W), ((1, 3), (3, 4))),
    ((TILE_H + 1, TILE_W - 1), ((3, 3), (1, 1)))) for B, C in pairs]
PARITY_CONTENTS = ('noise', 'blob')
CAP, FLOOR = 2e-5, 2.0 ** -21


def needs_reference():
    if not reference.available():
        pytest.skip('reference sources not staged: run oracle/make_ref.py (or __graft_entry__.build()) where the reference checkout exists')


@functools.lru_cache(maxsize=None)
def reference_error(dev):
    """e32: the reference's ops.blur on `dev` against the float64 restatement, the worst element over every parity case."""
    ref_blur = reference.modules().ops.blur
    worst = 0.0
    for B, C, H, W in SHAPES:
        for content in PARITY_CONTENTS:
            for white in (False, True):
                x = bu.permuted(bu.image(content, B, C, H, W, white), dev)
                for i in bu.ITERATIONS:
                    theirs = ref_blur(x, i, bu.WARMUP, white).cpu().double()
                    worst = max(worst, float((theirs - bu.blurred64(content, B, C, H, W, i, white)).abs().max()))
    return worst


def bound(dev):
    return min(2 * reference_error(dev) + FLOOR, CAP)


class Spy:
    """Records the keyword arguments of every _lib.call_struct call, by entry name."""

    def __init__(self, monkeypatch):
        self.calls = []
        real = _lib.call_struct

        def recorded(fname, struct_name, stream, *extra, **kw):
            self.calls.append((fname, stream, dict(kw)))
            return real(fname, struct_name, stream, *extra, **kw)
        monkeypatch.setattr(_lib, 'call_struct', recorded)

    def of(self, fname):
        return [(stream, kw) for name, stream, kw in self.calls if name == fname]


def test_tile_constants():
    """The tile this file places its sizes around is the kernel's, and the Python wrapper states the same limits."""
    from nerf_from_image_amd import ops
    src = open(os.path.join(os.path.dirname(_lib.LIBRARY), 'csrc', 'nfi_filter.inc')).read()
    m = re.search(r'constexpr int kFilterTileH = (\d+), kFilterTileW = (\d+), kFilterThreads = (\d+);', src)
    assert m and (int(m.group(1)), int(m.group(2))) == (TILE_H, TILE_W) == ops.FILTER_TILE
    assert int(re.search(r'constexpr int kFilterMaxRadius = (\d+);', src).group(1)) == ops.FILTER_MAX_RADIUS == 30


@pytest.mark.gpu
def test_the_reference_on_this_gpu_is_within_its_cpu_figure(gpu_device):
    """Not a condition on the kernel: reports e32 of this GPU's library convolution.  The bound is capped whatever it is."""
    needs_reference()
    e32 = reference_error(gpu_device)
    print('e32 (reference ops.blur on the GPU against float64, %d parity cases): %.3e; bound %.3e' % (
        len(SHAPES) * len(PARITY_CONTENTS) * 2 * len(bu.ITERATIONS), e32, bound(gpu_device)))
    assert e32 == e32 and bound(gpu_device) <= CAP


@pytest.mark.gpu
@pytest.mark.parametrize('B,C,H,W', SHAPES)
def test_blur_against_float64_in_both_layouts(gpu_device, B, C, H, W):
    from nerf_from_image_amd import filters
    needs_reference()
    tol = bound(gpu_device)
    worst = 0.0
    for content in PARITY_CONTENTS:
        for white in (False, True):
            x = bu.image(content, B, C, H, W, white)
            for name, xd in bu.layouts(x, gpu_device):
                for i in bu.ITERATIONS:
                    got = filters.blur(xd, i, bu.WARMUP, white)
                    assert got.shape == (B, C, H, W) and got.dtype == torch.float32 and got.is_contiguous() and got.device == xd.device
                    err = float((got.cpu().double() - bu.blurred64(content, B, C, H, W, i, white)).abs().max())
                    worst = max(worst, err)
                    assert err <= tol, (content, white, name, i, err, tol)
    print('blur parity %s: worst %.3e (e32 %.3e, bound %.3e)' % ((B, C, H, W), worst, reference_error(gpu_device), tol))


@pytest.mark.gpu
@pytest.mark.parametrize('H,W', [(5, 9), (37, 53), (TILE_H + 1, TILE_W - 1), (128, 128)])
def test_impulse_response(gpu_device, H, W):
    """A single 1.0 on zeros, black background: the output is f (x) f around it - every element within 1e-5 relative + 1e-12
    of float64, the outermost f[-r] f[-r] included - exactly 0.0 farther than r away, and cut off at the image's edge."""
    from nerf_from_image_amd import filters
    B, C = 1, 3
    ys, xs = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    for place in bu.IMPULSE_PLACES:
        iy, ix = bu.impulse_at(place, H, W)
        x = bu.image('impulse_' + place, B, C, H, W, False)
        for name, xd in bu.layouts(x, gpu_device):
            for i in bu.ITERATIONS:
                sigma, r = bu.schedule(i)
                f = bu.taps_ref(sigma, r, torch.float64)
                dy, dx = iy - ys, ix - xs                                       # out[y,x] = f[iy - y + r] f[ix - x + r]
                inside = (dy.abs() <= r) & (dx.abs() <= r)
                want = torch.where(inside, f[(dy + r).clamp(0, 2 * r)] * f[(dx + r).clamp(0, 2 * r)], torch.zeros((), dtype=torch.float64))
                assert float((want - bu.blurred64('impulse_' + place, B, C, H, W, i, False)[0, 0]).abs().max()) <= 1e-15
                got = filters.blur(xd, i, bu.WARMUP, False).cpu()
                for c in range(C):
                    g = got[0, c].double()
                    assert bool((g[~inside] == 0.0).all()), (place, name, i, c)
                    assert bool(((g - want).abs() <= 1e-5 * want.abs() + 1e-12).all()), (place, name, i, c, float((g - want).abs().max()))
                if iy - r >= 0 and ix - r >= 0:                                 # the outermost product is inside the image
                    assert float(got[0, 0, iy - r, ix - r]) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize('n', [3, 7, 61])
def test_filt2d_with_asymmetric_taps(gpu_device, n):
    """Random taps of no symmetry show a flipped or transposed pass.  Bound: max(2 x the float32 restatement's own worst
    distance to float64 on the same inputs, 2^-21) - computed on the CPU, here."""
    from nerf_from_image_amd import filters
    taps = bu.asymmetric_taps(n)
    for B, C, H, W in ((2, 3, 37, 53), (1, 4, TILE_H + 1, TILE_W - 1), (1, 1, 5, 9)):
        x = bu.image('noise', B, C, H, W, False)
        want = bu.filt_ref(x.double(), taps.double())
        tol = max(2 * float((bu.filt_ref(x, taps).double() - want).abs().max()), FLOOR)
        for wrong in (bu.filt_ref(x.double(), taps.double(), flip=True), bu.filt_ref(x.double().transpose(2, 3), taps.double().flip(0)).transpose(2, 3)):
            assert float((wrong - want).abs().max()) > 100 * tol          # the bound does tell a flipped pass apart
        for name, xd in bu.layouts(x, gpu_device):
            got = filters.filt2d(xd, taps.to(gpu_device))
            assert got.shape == x.shape and got.is_contiguous()
            err = float((got.cpu().double() - want).abs().max())
            assert err <= tol, (n, (B, C, H, W), name, err, tol)


def float64_gradient(x, cot, fn):
    xg = x.double().requires_grad_()
    grad, = torch.autograd.grad(fn(xg), xg, cot.double())
    return grad


@pytest.mark.gpu
@pytest.mark.parametrize('B,C,H,W', [(1, 3, 5, 9), (3, 4, 37, 53), (1, 4, TILE_H + 1, TILE_W - 1), (3, 4, 128, 128)])
def test_blur_gradient(gpu_device, B, C, H, W):
    """The image gradient of a seeded cotangent, image and cotangent in either layout, against float64 autograd of the
    restatement under the parity bound; the same bits for both backgrounds; create_graph=True raises."""
    from nerf_from_image_amd import filters
    needs_reference()
    tol = bound(gpu_device)
    x = bu.image('noise', B, C, H, W, False)
    cot = bu.image('noise', B, C, H, W, True)
    for i in bu.ITERATIONS:
        want = float64_gradient(x, cot, lambda t: bu.blur_ref(t, i, bu.WARMUP, True, torch.float64))
        seen = []
        for xname, xd in bu.layouts(x, gpu_device):
            for cname, cd in bu.layouts(cot, gpu_device):
                for white in (False, True):
                    leaf = xd.detach().requires_grad_()
                    grad, = torch.autograd.grad(filters.blur(leaf, i, bu.WARMUP, white), leaf, cd)
                    assert grad.shape == x.shape and grad.dtype == torch.float32
                    err = float((grad.cpu().double() - want).abs().max())
                    assert err <= tol, (i, xname, cname, white, err, tol)
                    seen.append(grad)
        assert all(torch.equal(g, seen[0]) for g in seen[1:]), i
    leaf = x.to(gpu_device).requires_grad_()
    with pytest.raises(RuntimeError, match='first-order only'):
        torch.autograd.grad(filters.blur(leaf, 0, bu.WARMUP, True), leaf, cot.to(gpu_device), create_graph=True)


@pytest.mark.gpu
def test_filt2d_gradient_with_asymmetric_taps(gpu_device):
    from nerf_from_image_amd import filters
    B, C, H, W = 2, 3, 37, 53
    x, cot = bu.image('noise', B, C, H, W, False), bu.image('noise', B, C, H, W, True)
    for n in (3, 7, 61):
        taps = bu.asymmetric_taps(n)
        want = float64_gradient(x, cot, lambda t: bu.filt_ref(t, taps.double()))
        x32 = x.clone().requires_grad_()
        g32, = torch.autograd.grad(bu.filt_ref(x32, taps), x32, cot)
        tol = max(2 * float((g32.double() - want).abs().max()), FLOOR)
        for xname, xd in bu.layouts(x, gpu_device):
            for cname, cd in bu.layouts(cot, gpu_device):
                leaf = xd.detach().requires_grad_()
                grad, = torch.autograd.grad(filters.filt2d(leaf, taps.to(gpu_device)), leaf, cd)
                err = float((grad.cpu().double() - want).abs().max())
                assert err <= tol, (n, xname, cname, err, tol)


@pytest.mark.gpu
@pytest.mark.parametrize('side_stream', [False, True])
def test_one_launch_forward_one_backward_on_the_callers_stream(gpu_device, monkeypatch, side_stream):
    """One blur is exactly one nfi_separable_filter call with null taps and the image's own pointer in its own layout; one
    backward is exactly one more, flipped, with background 0, reading the gradient in place; both on the current stream."""
    from nerf_from_image_amd import filters
    B, C, H, W = 3, 4, 37, 53
    x = bu.permuted(bu.image('blob', B, C, H, W, True), gpu_device).requires_grad_()
    cot = bu.permuted(bu.image('noise', B, C, H, W, True), gpu_device)
    want = filters.blur(x.detach(), 6250, bu.WARMUP, True)
    want_grad, = torch.autograd.grad(filters.blur(x, 6250, bu.WARMUP, True), x, cot)
    torch.cuda.synchronize(gpu_device)
    stream = torch.cuda.Stream(device=gpu_device) if side_stream else torch.cuda.current_stream(gpu_device)
    spy = Spy(monkeypatch)
    with torch.cuda.device(gpu_device), torch.cuda.stream(stream):
        out = filters.blur(x, 6250, bu.WARMUP, True)
        assert [name for name, _, _ in spy.calls] == ['nfi_separable_filter']
        grad, = torch.autograd.grad(out, x, cot)
    stream.synchronize()
    assert [name for name, _, _ in spy.calls] == ['nfi_separable_filter'] * 2
    (s_fwd, fwd), (s_bwd, bwd) = spy.of('nfi_separable_filter')
    assert s_fwd == s_bwd == stream.cuda_stream
    assert side_stream == (stream.cuda_stream != torch.cuda.default_stream(gpu_device).cuda_stream)
    sigma, r = bu.schedule(6250)
    assert fwd['taps'] is None and bwd['taps'] is None and fwd['radius'] == bwd['radius'] == r == 15 and fwd['sigma'] == bwd['sigma'] == sigma
    assert (fwd['image'].data_ptr(), fwd['layout'], fwd['background'], fwd['flip']) == (x.data_ptr(), 1, 1.0, 0)
    assert (bwd['image'].data_ptr(), bwd['layout'], bwd['background'], bwd['flip']) == (cot.data_ptr(), 1, 0.0, 1)
    assert torch.equal(out, want) and torch.equal(grad, want_grad)


@pytest.mark.gpu
def test_a_layout_that_is_neither_is_copied(gpu_device, monkeypatch):
    """A [:, :3] slice of four channels-last channels is dense in neither layout: it is copied to [B,C,H,W], same result."""
    from nerf_from_image_amd import filters
    x = bu.permuted(bu.image('noise', 2, 4, 37, 53, False), gpu_device)
    sliced = x[:, :3]
    assert not sliced.is_contiguous() and not sliced.permute(0, 2, 3, 1).is_contiguous()
    spy = Spy(monkeypatch)
    got = filters.blur(sliced, 11000, bu.WARMUP, True)
    (_, kw), = spy.of('nfi_separable_filter')
    assert kw['image'].data_ptr() != sliced.data_ptr() and kw['image'].is_contiguous() and kw['layout'] == 0
    assert torch.equal(got, filters.blur(x, 11000, bu.WARMUP, True)[:, :3])


@pytest.mark.gpu
def test_twenty_launches_give_the_same_bits(gpu_device):
    from nerf_from_image_amd import filters
    x = bu.permuted(bu.image('noise', 3, 4, 128, 128, True), gpu_device)
    for i in (0, 12083):
        first = filters.blur(x, i, bu.WARMUP, True)
        for _ in range(19):
            assert torch.equal(filters.blur(x, i, bu.WARMUP, True), first)


@pytest.mark.gpu
@pytest.mark.parametrize('white', [False, True])
def test_drop_in_for_the_real_phase_of_the_discriminator_step(gpu_device, white):
    """run.py:1090-1096 with filters.blur in place of the reference's ops.blur: the blurred batch, and the gradient that
    reaches it from a small fixed conv, agree with the reference's sequence under the parity bound (value) and under the
    same bound scaled by the conv's gain (gradient: it does not pass through the blur, so only the values' difference
    enters), plus 1e-5 of the gradient's size for the two float32 convs of 36 terms each (2 x 36 x 2^-24 = 4.3e-6)."""
    from nerf_from_image_amd import filters
    needs_reference()
    ref_blur = reference.modules().ops.blur
    B, C, H, W = 4, 4, 128, 128
    g = torch.Generator().manual_seed(5)
    weight = torch.randn(2, C, 3, 3, generator=g).to(gpu_device)
    target = bu.image('blob', B, C, H, W, white).permute(0, 2, 3, 1).contiguous().to(gpu_device)       # [B,H,W,C] as sample_batch gives it
    tol = bound(gpu_device)
    for i in (0, 6250, 12083, 12084):
        results = []
        for blur in (filters.blur, ref_blur):
            img = blur(target.permute(0, 3, 1, 2), i, bu.WARMUP, white).permute(0, 2, 3, 1)
            img = img.requires_grad_()
            disc = torch.nn.functional.conv2d(img.permute(0, 3, 1, 2), weight, padding=1)
            grad, = torch.autograd.grad((disc * disc).sum(), img)
            assert img.shape == (B, H, W, C) and grad.shape == (B, H, W, C)
            results.append((img.detach(), grad))
        (ours, g_ours), (theirs, g_theirs) = results
        assert float((ours - theirs).abs().max()) <= tol + reference_error(gpu_device), i
        # d/d img of sum(conv(img)^2) = 2 conv^T(conv(img)): linear in img with gain <= 2 (sum |w|)^2
        gain = 2 * float(weight.abs().sum()) ** 2
        assert float((g_ours - g_theirs).abs().max()) <= gain * (tol + reference_error(gpu_device)) + 1e-5 * float(g_theirs.abs().max()), i
