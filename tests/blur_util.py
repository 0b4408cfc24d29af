"""What tests/test_blur_abi.py and tests/test_blur_gpu.py share: a plain-torch restatement of lib/ops.py:29-55 (blur, and
filt2d with a 1-D kernel) that runs in a given dtype - float64 is the yardstick - the seeded inputs, and the cases.

The restatement is written from the formulas, not from the reference's text: the schedule in Python doubles
(sigma = max(1 - i / warmup, 0) * 10, r = floor(3 sigma), identity at r = 0), taps exp2(-(k / sigma)^2) for k = -r .. r
divided by their sum, two zero-padded 1-D cross-correlations (rows, then columns) of image - background, + background."""
import functools
import math

import torch
import torch.nn.functional as F

WARMUP = 12500
ITERATIONS = (0, 6250, 11000, 12083)          # r = 30, 15, 3, 1


def schedule(i, warmup=WARMUP):
    sigma = max(1 - i / warmup, 0) * 10
    return sigma, int(math.floor(sigma * 3))


def taps_ref(sigma, r, dtype):
    k = torch.arange(-r, r + 1, dtype=dtype)
    f = torch.exp2(-(k / sigma) ** 2)
    return f / f.sum()


def filt_ref(im, taps, flip=False):
    """Zero-padded same-size cross-correlation of im [B,C,H,W] with taps (x) taps, in im's dtype: out[y,x] =
    sum_{a,b} f[a] f[b] im[y+a-r, x+b-r].  flip applies the taps reversed (the adjoint)."""
    f = taps.to(im.dtype)
    if flip:
        f = f.flip(0)
    r = f.shape[0] // 2
    b, c, h, w = im.shape
    planes = im.reshape(b * c, 1, h, w)
    rows = F.conv2d(planes, f.view(1, 1, 1, -1), padding=(0, r))
    both = F.conv2d(rows, f.view(1, 1, -1, 1), padding=(r, 0))
    return both.view(b, c, h, w)


def blur_ref(image, i, warmup, white_background, dtype):
    """blur in `dtype`; returns `image` itself where the radius is 0, as the reference does."""
    sigma, r = schedule(i, warmup)
    if r == 0:
        return image
    bg = 1.0 if white_background else 0.0
    return filt_ref(image.to(dtype) - bg, taps_ref(sigma, r, dtype)) + bg


def seed_of(*parts):
    s = 29
    for p in parts:
        for ch in str(p):
            s = (s * 131 + ord(ch)) % 2147483629
    return s


def blob(B, C, H, W, g, background):
    """A smooth bump per image and channel on a flat background of 0 or 1."""
    yy = torch.linspace(-1, 1, H).view(1, 1, H, 1)
    xx = torch.linspace(-1, 1, W).view(1, 1, 1, W)
    cy, cx = torch.rand(B, 1, 1, 1, generator=g) - 0.5, torch.rand(B, 1, 1, 1, generator=g) - 0.5
    width = 0.15 + 0.25 * torch.rand(B, 1, 1, 1, generator=g)
    bump = torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * width ** 2))
    bump = torch.where(bump < 0.05, torch.zeros(()), bump)
    colour = torch.rand(B, C, 1, 1, generator=g)
    return (background + (colour - background) * bump).float()


IMPULSE_PLACES = ('corner', 'edge', 'interior')


def impulse_at(place, H, W):
    return {'corner': (0, W - 1), 'edge': (H // 2, 0), 'interior': (H // 2, W // 2)}[place]


CONTENTS = ('noise', 'blob') + tuple('impulse_' + p for p in IMPULSE_PLACES)


@functools.lru_cache(maxsize=None)
def image(content, B, C, H, W, white_background):
    """float32 [B,C,H,W]: uniform noise in [-1,1]; a blob on the flat background the blur is told about; a single 1.0 on
    zeros (every image and channel) at a corner, on an edge, in the interior."""
    g = torch.Generator().manual_seed(seed_of(content, B, C, H, W, white_background))
    if content == 'noise':
        return torch.rand(B, C, H, W, generator=g) * 2 - 1
    if content == 'blob':
        return blob(B, C, H, W, g, 1.0 if white_background else 0.0)
    x = torch.zeros(B, C, H, W)
    y, xx = impulse_at(content[len('impulse_'):], H, W)
    x[:, :, y, xx] = 1.0
    return x


@functools.lru_cache(maxsize=None)
def blurred64(content, B, C, H, W, i, white_background):
    """The float64 yardstick of one case.  Computed once; callers must not modify it."""
    return blur_ref(image(content, B, C, H, W, white_background), i, WARMUP, white_background, torch.float64)


def permuted(t, dev):
    """The same values dense as [B,H,W,C] on dev, seen as [B,C,H,W] through permute(0,3,1,2): what run.py hands over."""
    return t.permute(0, 2, 3, 1).contiguous().to(dev).permute(0, 3, 1, 2)


def layouts(t, dev):
    return (('BCHW', t.to(dev)), ('BHWC', permuted(t, dev)))


def asymmetric_taps(n):
    """Seeded random taps of odd length n, of both signs and no symmetry."""
    g = torch.Generator().manual_seed(seed_of('taps', n))
    return torch.randn(n, generator=g) / math.sqrt(n)
