"""What tests/test_ssim_abi.py and tests/test_ssim_gpu.py share: the restatement of lib/metrics.py:48-76 in plain torch
(five avg_pool2d - float64 is the oracle, float32 the reference's own arithmetic for float32 inputs and the yardstick), the
seeded inputs, and the references of every case, computed once."""
import functools

import torch
import torch.nn.functional as F

C1, C2, WIN = 1e-4, 9e-4, 7


def ssim_map_ref(x, y, dtype, clamp=True):
    """The cropped SSIM map [B,3,H-6,W-6] of x, y [B,3,H,W] after the clamp to [0,1], carried out in `dtype`.
    clamp=False leaves the clamp out: what an implementation that forgot it would give."""
    x, y = x.to(dtype), y.to(dtype)
    if clamp:
        x, y = x.clamp(0, 1), y.clamp(0, 1)
    u = lambda t: F.avg_pool2d(t, WIN, 1)
    ux, uy, uxx, uyy, uxy = u(x), u(y), u(x * x), u(y * y), u(x * y)
    norm = WIN * WIN / (WIN * WIN - 1.0)
    vx, vy, vxy = norm * (uxx - ux * ux), norm * (uyy - uy * uy), norm * (uxy - ux * uy)
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def ssim_ref(x, y, dtype, clamp=True):
    """(per-image value [B], map [B,3,H-6,W-6]): the mean over window centres per channel, then over the channels."""
    m = ssim_map_ref(x, y, dtype, clamp)
    return m.mean(dim=(2, 3)).mean(dim=1), m


def seed_of(*parts):
    s = 23
    for p in parts:
        for ch in str(p):
            s = (s * 131 + ord(ch)) % 2147483629
    return s


def blob(B, H, W, g, background):
    """A smooth bump per image and channel, of random centre, width and colour, on a flat background of 0 or 1."""
    yy = torch.linspace(-1, 1, H).view(1, 1, H, 1)
    xx = torch.linspace(-1, 1, W).view(1, 1, 1, W)
    cy, cx = (torch.rand(B, 1, 1, 1, generator=g) - 0.5), (torch.rand(B, 1, 1, 1, generator=g) - 0.5)
    width = 0.15 + 0.25 * torch.rand(B, 1, 1, 1, generator=g)
    bump = torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * width ** 2))
    bump = torch.where(bump < 0.05, torch.zeros(()), bump)               # exactly flat away from the bump
    colour = torch.rand(B, 3, 1, 1, generator=g)
    return (background + (colour - background) * bump).float()


CONTENTS = ('noise', 'blob_white', 'blob_black', 'identical', 'ones_vs_blob')


@functools.lru_cache(maxsize=None)
def case(content, B, H, W):
    """dict(pred, target float32 [B,3,H,W] in [0,1]; value64 [B], map64; value32 / map32: the float32 restatement)."""
    g = torch.Generator().manual_seed(seed_of(content, B, H, W))
    noisy = lambda t: (t + 0.05 * torch.randn(t.shape, generator=g)).clamp(0, 1)
    if content == 'noise':
        target = torch.rand(B, 3, H, W, generator=g)
        pred = noisy(target)
    elif content == 'blob_white':
        target = blob(B, H, W, g, 1.0)
        pred = noisy(target)
    elif content == 'blob_black':
        target = blob(B, H, W, g, 0.0)
        pred = noisy(target)
    elif content == 'identical':
        target = blob(B, H, W, g, 1.0) * (0.5 + 0.5 * torch.rand(B, 3, H, W, generator=g))
        pred = target.clone()
    else:
        target = blob(B, H, W, g, 1.0)
        pred = torch.ones(B, 3, H, W)
    v64, m64 = ssim_ref(pred, target, torch.float64)
    v32, m32 = ssim_ref(pred, target, torch.float32)
    return dict(pred=pred, target=target, value64=v64, map64=m64, value32=v32, map32=m32)
