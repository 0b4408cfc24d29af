"""metrics.ssim(..., reduction='none') against the float32 avg_pool2d restatement of lib/metrics.py:48-76 a user without it
would write with PyTorch-ROCm on the same GPU: HIP events on the launch stream, the two contenders alternating inside one
process:   python tools/bench_ssim.py [iterations]
  B = 16 at 3 x 128 x 128 and 3 x 256 x 256, both inputs dense [B,3,H,W] or both dense [B,H,W,3] behind a permute.
  Both contenders include their range check and its read of the flag (the reference asserts it per call).  Parity: the
  largest distance of either contender's per-image value to the same restatement in float64, also on the GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from nerf_from_image_amd import _lib  # noqa: E402
if os.environ.get('NFI_PROBE_LIBRARY'):          # a variant build, as tools/bench_regulariser.py
    _lib.LIBRARY = os.environ['NFI_PROBE_LIBRARY']
from nerf_from_image_amd import metrics  # noqa: E402


def restatement(pred, target, dtype=torch.float32):
    """lib/metrics.py:48-76 with torch ops: range check, clamp, five 7 x 7 box means, the mean over the window centres."""
    assert bool(((pred > -0.1) & (pred < 1.1) & (target > -0.1) & (target < 1.1)).all()), 'Range check failed'
    x, y = pred.to(dtype).clamp(0, 1), target.to(dtype).clamp(0, 1)
    u = lambda t: F.avg_pool2d(t, 7, 1)
    ux, uy, uxx, uyy, uxy = u(x), u(y), u(x * x), u(y * y), u(x * y)
    vx, vy, vxy = (49 / 48) * (uxx - ux * ux), (49 / 48) * (uyy - uy * uy), (49 / 48) * (uxy - ux * uy)
    s = ((2 * ux * uy + 1e-4) * (2 * vxy + 9e-4)) / ((ux * ux + uy * uy + 1e-4) * (vx + vy + 9e-4))
    return s.mean(dim=(2, 3)).mean(dim=1)


def alternate(fns, n, warm=5):
    """Median ms of each of fns, called in turn n times (after `warm` rounds), and the last outputs."""
    for _ in range(warm):
        outs = [f() for f in fns]
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(n):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); outs[i] = f(); b.record()
            times[i].append((a, b))
    torch.cuda.synchronize()
    return [sorted(a.elapsed_time(b) for a, b in t)[n // 2] for t in times], outs


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    B = 16
    for R in (128, 256):
        # a render-like pair: a smooth shape on a white background and a noisy copy of it
        yy, xx = torch.linspace(-1, 1, R).view(1, 1, R, 1), torch.linspace(-1, 1, R).view(1, 1, 1, R)
        shape = torch.exp(-(yy ** 2 + xx ** 2) / (2 * (0.2 + 0.2 * torch.rand(B, 1, 1, 1, generator=g)) ** 2))
        target = (1 + (torch.rand(B, 3, 1, 1, generator=g) - 1) * shape).float()
        pred = (target + 0.05 * torch.randn(B, 3, R, R, generator=g)).clamp(0, 1)
        for layout in ('[B,3,H,W]', '[B,H,W,3]'):
            if layout == '[B,3,H,W]':
                p, t = pred.to(dev), target.to(dev)
            else:
                p, t = (v.permute(0, 2, 3, 1).contiguous().to(dev).permute(0, 3, 1, 2) for v in (pred, target))
            (t_hip, t_torch), (ours, theirs) = alternate([lambda: metrics.ssim(p, t, reduction='none'), lambda: restatement(p, t)], n)
            again = metrics.ssim(p, t, reduction='none')
            ref = restatement(p, t, torch.float64)
            print('ssim B = %d, 3 x %d x %d, %s: HIP %.3f ms, float32 avg_pool2d restatement %.3f ms, ratio %.2f; distance to the '
                  'float64 restatement: HIP %.2e, float32 restatement %.2e; repeat bit-identical: %s' % (
                      B, R, R, layout, t_hip, t_torch, t_torch / t_hip, float((ours.double() - ref).abs().max()),
                      float((theirs.double() - ref).abs().max()), torch.equal(again, ours)))


if __name__ == '__main__':
    main()
