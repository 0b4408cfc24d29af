"""metrics.ssim / ops.image_ssim (csrc/nfi_neighbours.inc, ssim_tile_kernel + ssim_finish_kernel) on the GPU against the
float64 restatement of lib/metrics.py:48-76 (tests/ssim_util.py, pinned to scipy's filter by tests/test_ssim_abi.py).

Sizes: 7 x 7 (one window), one-window strips 7 x 40 and 40 x 7, 8 x 13, 37 x 29, and around the kernel's tile of 16 x 32
window centres - 15 x 31, 16 x 32, 17 x 33 and 23 x 39 centres, i.e. images of 21 x 37, 22 x 38, 23 x 39 and 29 x 45 (one
short of the tile edge, on it, 1 and 7 beyond it) - and 128 x 128 (8 x 4 tiles); B = 1, 2 and 5.

The bound is not a number from a run of the kernel: it is max(2 x the float32 restatement's own worst distance to float64
over all of this file's cases, 4 x 2^-23), for the per-image value and, with the per-pixel maximum, for the map.  The
factor 2 is for the kernel's summation order, which is not the restatement's; the floor is there because the restatement
can be exact, as it is on identical images."""
import functools

import numpy as np
import pytest
import torch

from ssim_util import CONTENTS, case, ssim_ref

TILE_H, TILE_W = 16, 32
SIZES = [(1, 7, 7), (2, 7, 40), (2, 40, 7), (5, 8, 13), (2, 37, 29),
         (1, TILE_H - 1 + 6, TILE_W - 1 + 6), (2, TILE_H + 6, TILE_W + 6), (2, TILE_H + 1 + 6, TILE_W + 1 + 6), (1, TILE_H + 7 + 6, TILE_W + 7 + 6),
         (2, 128, 128)]
FLOOR = 4 * 2.0 ** -23


@functools.lru_cache(maxsize=None)
def bounds():
    """(value bound, map bound, value yardstick, map yardstick) over every case of this file, on the CPU."""
    value = max(float((case(c, *s)['value32'].double() - case(c, *s)['value64']).abs().max()) for c in CONTENTS for s in SIZES)
    pixel = max(float((case(c, *s)['map32'].double() - case(c, *s)['map64']).abs().max()) for c in CONTENTS for s in SIZES)
    return max(2 * value, FLOOR), max(2 * pixel, FLOOR), value, pixel


def layouts(t, dev):
    """[B,3,H,W] dense, and the same values dense as [B,H,W,3] behind permute(0,3,1,2) (what run.py hands over)"""
    return (('BCHW', t.to(dev)), ('BHWC', t.permute(0, 2, 3, 1).contiguous().to(dev).permute(0, 3, 1, 2)))


class Spy:
    """Records the keyword arguments of every _lib.call_struct call, by entry name."""

    def __init__(self, monkeypatch):
        from nerf_from_image_amd import _lib
        self.calls = []
        real = _lib.call_struct

        def recorded(fname, struct_name, stream, *extra, **kw):
            self.calls.append((fname, stream, dict(kw)))
            return real(fname, struct_name, stream, *extra, **kw)
        monkeypatch.setattr(_lib, 'call_struct', recorded)

    def of(self, fname):
        return [(stream, kw) for name, stream, kw in self.calls if name == fname]


@pytest.mark.gpu
@pytest.mark.parametrize('B,H,W', SIZES)
def test_against_float64_in_both_layouts(gpu_device, B, H, W):
    """Every content at this size, pred and target in either layout (mixed too): per-image value and map within their
    bounds of float64; the map's shape, its per-channel means reproduce the value, and asking for it does not change a bit
    of the value; reduction='mean' is the mean of 'none' as [1]."""
    from nerf_from_image_amd import metrics, ops
    value_tol, map_tol, value_yard, map_yard = bounds()
    worst_v = worst_m = 0.0
    for content in CONTENTS:
        c = case(content, B, H, W)
        for pname, p in layouts(c['pred'], gpu_device):
            for tname, t in layouts(c['target'], gpu_device):
                per = metrics.ssim(p, t, reduction='none')
                assert per.shape == (B,) and per.dtype == torch.float32 and per.device == p.device
                ev = float((per.cpu().double() - c['value64']).abs().max())
                worst_v = max(worst_v, ev)
                assert ev <= value_tol, (content, pname, tname, ev, value_tol)
                value, smap, flag = ops.image_ssim(p, t, want_map=True)
                assert torch.equal(value, per) and int(flag) == 0
                assert smap.shape == (B, 3, H - 6, W - 6) and smap.is_contiguous()
                em = float((smap.cpu().double() - c['map64']).abs().max())
                worst_m = max(worst_m, em)
                assert em <= map_tol, (content, pname, tname, em, map_tol)
                from_map = smap.cpu().double().mean(dim=(2, 3)).mean(dim=1)
                assert float((from_map - per.cpu().double()).abs().max()) <= value_tol
                mean = metrics.ssim(p, t)
                assert mean.shape == (1,) and mean.dtype == torch.float32 and mean.device == p.device
                assert torch.equal(mean, per.mean(dim=0, keepdim=True))
                if content == 'identical':
                    assert float((per.cpu().double() - 1.0).abs().max()) <= value_tol, per
    print('ssim parity %s: value %.3e (float32 restatement %.3e, bound %.3e), map %.3e (float32 restatement %.3e, bound %.3e)' % (
        (B, H, W), worst_v, value_yard, value_tol, worst_m, map_yard, map_tol))


@pytest.mark.gpu
def test_channels_last_is_read_in_place_and_a_slice_is_copied(gpu_device, monkeypatch):
    """run.py's permute(0,3,1,2)[:, :3] / 2 + 0.5 of a [B,H,W,3] render is dense channels-last: the kernel gets the tensor's
    own pointer with layout 1 (and a dense [B,3,H,W] its own with layout 0).  A [:, :3] slice of four channels is dense in
    neither layout: it is copied, to layout 0, and gives the same value."""
    from nerf_from_image_amd import ops
    spy = Spy(monkeypatch)
    c = case('blob_white', 2, 37, 29)
    (_, p0), (_, p1) = layouts(c['pred'], gpu_device)
    (_, t0), (_, t1) = layouts(c['target'], gpu_device)
    assert not p1.is_contiguous() and p1.permute(0, 2, 3, 1).is_contiguous()
    want, _, _ = ops.image_ssim(p0, t0)
    got, _, _ = ops.image_ssim(p1, t0)
    rgba = torch.cat([c['pred'], torch.rand(2, 1, 37, 29)], dim=1).permute(0, 2, 3, 1).contiguous().to(gpu_device)      # [B,H,W,4]
    sliced = rgba.permute(0, 3, 1, 2)[:, :3]
    assert not sliced.is_contiguous() and not sliced.permute(0, 2, 3, 1).is_contiguous()
    from_slice, _, _ = ops.image_ssim(sliced, t1)
    (_, a), (_, b), (_, s) = spy.of('nfi_image_ssim')
    assert (a['pred'].data_ptr(), a['pred_layout'], a['target'].data_ptr(), a['target_layout']) == (p0.data_ptr(), 0, t0.data_ptr(), 0)
    assert (b['pred'].data_ptr(), b['pred_layout'], b['target'].data_ptr(), b['target_layout']) == (p1.data_ptr(), 1, t0.data_ptr(), 0)
    assert s['pred'].data_ptr() != sliced.data_ptr() and s['pred'].is_contiguous() and s['pred_layout'] == 0
    assert (s['target'].data_ptr(), s['target_layout']) == (t1.data_ptr(), 1)
    value_tol = bounds()[0]
    for v in (want, got, from_slice):
        assert float((v.cpu().double() - c['value64']).abs().max()) <= value_tol
    assert torch.equal(from_slice, want)          # the copy holds the same values in layout 0: the same arithmetic


@pytest.mark.gpu
def test_repeats_and_does_not_depend_on_the_batch(gpu_device):
    """No tolerance: two launches on the same input are bit-identical (value and map), and image i of a batch of 5 has the
    bits it has alone and in last position of another batch."""
    from nerf_from_image_amd import ops
    for content, H, W in (('noise', 37, 29), ('blob_white', 29, 45), ('blob_black', 128, 128)):
        c = case(content, 5, H, W)
        p, t = c['pred'].to(gpu_device), c['target'].to(gpu_device)
        first, first_map, _ = ops.image_ssim(p, t, want_map=True)
        again, again_map, _ = ops.image_ssim(p, t, want_map=True)
        assert torch.equal(first, again) and torch.equal(first_map, again_map)
        for i in range(5):
            alone, _, _ = ops.image_ssim(p[i:i + 1], t[i:i + 1])
            assert torch.equal(alone[0], first[i]), (content, i)
            order = [j for j in range(5) if j != i] + [i]
            last, _, _ = ops.image_ssim(p[order].contiguous(), t[order].contiguous())
            assert torch.equal(last[4], first[i]), (content, i)


BAD_VALUES = {'1.1': np.float32(1.1), '-0.1': np.float32(-0.1), 'nan': np.float32('nan')}


@pytest.mark.gpu
def test_range_check(gpu_device):
    """lib/metrics.py:22-27 on both inputs: one element of exactly float32(1.1), float32(-0.1) or NaN - the last element of
    the last image or a corner pixel, in either input and either layout - fails the check; check_range=False returns without
    a flag; 1.05 and -0.05 pass and are clamped."""
    from nerf_from_image_amd import metrics, ops
    B, H, W = 2, 29, 45
    c = case('blob_black', B, H, W)
    places = {'last element': (B - 1, 2, H - 1, W - 1), 'corner': (0, 0, 0, W - 1)}
    for which in ('pred', 'target'):
        for place, idx in places.items():
            for label, value in BAD_VALUES.items():
                t = {k: c[k].clone() for k in ('pred', 'target')}
                t[which][idx] = float(value)
                for (pname, p), (tname, tt) in zip(layouts(t['pred'], gpu_device), layouts(t['target'], gpu_device)):
                    with pytest.raises(AssertionError, match='Range check failed'):
                        metrics.ssim(p, tt, reduction='none')
                    with pytest.raises(AssertionError, match='Range check failed'):
                        metrics.ssim(p, tt)
                p, tt = t['pred'].to(gpu_device), t['target'].to(gpu_device)
                value, _, flag = ops.image_ssim(p, tt, check_range=False)
                assert flag is None and value.shape == (B,)
                assert int(ops.image_ssim(p, tt)[2]) == 1
    soft = {k: c[k].clone() for k in ('pred', 'target')}
    soft['pred'][:, :, :8, :8], soft['pred'][:, :, H - 8:, W - 8:] = 1.05, -0.05           # two corner patches, corners included
    soft['target'][:, :, 10:18, 20:28], soft['target'][:, :, H - 8:, :8] = -0.05, 1.05
    want, _ = ssim_ref(soft['pred'], soft['target'], torch.float64)
    unclamped, _ = ssim_ref(soft['pred'], soft['target'], torch.float64, clamp=False)
    assert float((want - unclamped).abs().min()) > 10 * bounds()[0]           # in every image the clamp matters
    got = metrics.ssim(soft['pred'].to(gpu_device), soft['target'].to(gpu_device), reduction='none')
    assert float((got.cpu().double() - want).abs().max()) <= bounds()[0]


class ReadCounter:
    """Counts the device-to-host reads of int32 tensors (the range flags): .item(), .tolist(), .cpu(), int() and bool()."""

    def __init__(self, monkeypatch):
        self.reads = 0
        for name in ('item', 'tolist', 'cpu', '__int__', '__bool__'):
            monkeypatch.setattr(torch.Tensor, name, self.counting(getattr(torch.Tensor, name)))
        self.depth = 0

    def counting(self, real):
        def counted(t, *a, **kw):
            outermost = self.depth == 0
            if outermost and t.is_cuda and t.dtype == torch.int32:
                self.reads += 1
            self.depth += 1
            try:
                return real(t, *a, **kw)
            finally:
                self.depth -= 1
        return counted


@pytest.mark.gpu
def test_psnr_ssim_iou(gpu_device, monkeypatch):
    """The report's three vectors equal the three separate calls bit for bit, come from two launches, and the two range
    flags reach the host in one read; a bad value in the images or in a mask fails the check."""
    from nerf_from_image_amd import metrics
    B, H, W = 5, 37, 29
    c = case('blob_white', B, H, W)
    g = torch.Generator().manual_seed(3)
    p, t = c['pred'].to(gpu_device), c['target'].to(gpu_device)
    mp, mr = torch.rand(B, 1, H, W, generator=g).to(gpu_device), torch.rand(B, 1, H, W, generator=g).to(gpu_device)
    want = (metrics.psnr(p, t, reduction='none'), metrics.ssim(p, t, reduction='none'), metrics.iou(mp, mr, reduction='none'))
    with monkeypatch.context() as m:
        spy, reads = Spy(m), ReadCounter(m)
        got = metrics.psnr_ssim_iou(p, t, mp, mr)
        assert reads.reads == 1, reads.reads
        assert sorted(name for name, _, _ in spy.calls) == ['nfi_image_metrics', 'nfi_image_ssim']
    for a, b in zip(got, want):
        assert a.shape == (B,) and torch.equal(a, b)
    for which in ('pred', 'mask'):
        bad_p, bad_m = p.clone(), mr.clone()
        (bad_p if which == 'pred' else bad_m).view(-1)[-1] = 1.5
        with pytest.raises(AssertionError, match='Range check failed'):
            metrics.psnr_ssim_iou(bad_p, t, mp, bad_m)


@pytest.mark.gpu
def test_runs_on_the_callers_stream_and_device(gpu_device, monkeypatch):
    """Under torch.cuda.device and a side stream the launch goes to that stream (the handle the entry is given), and the
    value is the default stream's."""
    from nerf_from_image_amd import metrics
    c = case('noise', 2, 37, 29)
    p, t = c['pred'].to(gpu_device), c['target'].to(gpu_device)
    want = metrics.ssim(p, t, reduction='none')
    torch.cuda.synchronize(gpu_device)
    spy = Spy(monkeypatch)
    side = torch.cuda.Stream(device=gpu_device)
    with torch.cuda.device(gpu_device), torch.cuda.stream(side):
        got = metrics.ssim(p, t, reduction='none')
        mean = metrics.ssim(p, t)
    side.synchronize()
    streams = [stream for stream, _ in spy.of('nfi_image_ssim')]
    assert streams == [side.cuda_stream, side.cuda_stream] and side.cuda_stream != torch.cuda.default_stream(gpu_device).cuda_stream
    assert got.device == p.device and torch.equal(got, want) and torch.equal(mean, want.mean(dim=0, keepdim=True))
