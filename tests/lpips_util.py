"""What tests/test_lpips_abi.py and tests/test_lpips_gpu.py share: a plain-torch restatement of the LPIPS distance head
(lib/metrics.py:104-110, 130-133; float64 is the oracle, float32 the yardstick of what float32 arithmetic itself loses), its
gradient by autograd, the seeded inputs, the shape grid and a five-tap stand-in for the VGG network.

    rx[b,p] = sqrt(sum_c x[b,c,p]^2)     xh = x / (rx + eps)        (eps added to the norm, not under the root)
    ry, yh likewise; y_normalized: yh = y as given
    out[b]  = (1 / (H W)) sum_p sum_c w[c] (xh[b,c,p] - yh[b,c,p])^2
"""
import copy
import functools

import torch
from torch import nn

EPS = 1e-10
TILE = 64                           # kLpipsTile of csrc/nfi_lpips.inc (test_lpips_gpu.test_tile_constants holds it to that)
RESIDENT = (64, 128)                # channel counts the kernels keep in registers
FLOOR = 4 * 2.0 ** -23


def normalize(x, eps=EPS):
    return x / (torch.sqrt(torch.sum(x * x, dim=1, keepdim=True)) + eps)


def head_ref(x, y, w, dtype, y_normalized=False, eps=EPS):
    """out [B] of one layer, carried out in `dtype`."""
    x, y, w = x.to(dtype), y.to(dtype), w.to(dtype)
    d = normalize(x, eps) - (y if y_normalized else normalize(y, eps))
    return (d * d * w.view(1, -1, 1, 1)).sum(dim=1).mean(dim=(1, 2))


def head_loops(x, y, w, y_normalized=False, eps=EPS):
    """The same, as explicit loops over images, pixels and channels in Python floats (float64)."""
    B, C, H, W = x.shape
    out = []
    for b in range(B):
        total = 0.0
        for i in range(H):
            for j in range(W):
                rx = sum(float(x[b, c, i, j]) ** 2 for c in range(C)) ** 0.5
                ry = sum(float(y[b, c, i, j]) ** 2 for c in range(C)) ** 0.5
                for c in range(C):
                    xh = float(x[b, c, i, j]) / (rx + eps)
                    yh = float(y[b, c, i, j]) if y_normalized else float(y[b, c, i, j]) / (ry + eps)
                    total += float(w[c]) * (xh - yh) ** 2
        out.append(total / (H * W))
    return torch.tensor(out, dtype=torch.float64)


def head_grads(x, y, w, g_out, dtype, y_normalized=False, eps=EPS):
    """(out, g_x, g_y) by autograd of the restatement in `dtype`."""
    xg, yg = x.detach().to(dtype, copy=True).requires_grad_(), y.detach().to(dtype, copy=True).requires_grad_()
    out = head_ref(xg, yg, w, dtype, y_normalized, eps)
    g_x, g_y = torch.autograd.grad(out, (xg, yg), g_out.to(dtype))
    return out.detach(), g_x, g_y


def seed_of(*parts):
    s = 29
    for p in parts:
        for ch in str(p):
            s = (s * 131 + ord(ch)) % 2147483629
    return s


CONTENTS = ('noise', 'near', 'identical', 'scaled_small', 'scaled_large')


def features(B, C, H, W, g, scale=1.0):
    """relu(randn) * scale with channel 0 raised: a real VGG tap always has a live channel, and without it a small C gives
    pixels that are zero across the channels, where the reference's gradient is NaN."""
    f = torch.relu(torch.randn(B, C, H, W, generator=g))
    f[:, 0] += 0.25 + 0.5 * torch.rand(B, H, W, generator=g)
    return (f * scale).float()


def cotangent(B, g):
    """Non-uniform, with a zero and a negative entry wherever the batch has room for them."""
    c = 0.5 + torch.rand(B, generator=g)
    if B >= 2:
        c[1] = -c[1]
    if B >= 3:
        c[2] = 0.0
    return c.float()


@functools.lru_cache(maxsize=None)
def case(content, B, C, H, W, y_normalized=False):
    """dict(x, y, w, g_out float32; out64, gx64, gy64: the float64 restatement; out32, gx32, gy32: the float32 one)."""
    g = torch.Generator().manual_seed(seed_of(content, B, C, H, W, y_normalized))
    scale = {'scaled_small': 1e-3, 'scaled_large': 1e3}.get(content, 1.0)
    x = features(B, C, H, W, g, scale)
    if content == 'identical':
        y = x.clone()
    else:
        amount = 1e-3 if content == 'near' else 0.5
        y = torch.relu(x + amount * scale * torch.randn(B, C, H, W, generator=g)).float()
        y[:, 0] = torch.maximum(y[:, 0], torch.full((), 0.125 * scale))
    if y_normalized:
        y = normalize(y.double()).float()
    w = ((0.5 + torch.rand(C, generator=g)) / C).float()
    g_out = cotangent(B, g)
    out64, gx64, gy64 = head_grads(x, y, w, g_out, torch.float64, y_normalized)
    out32, gx32, gy32 = head_grads(x, y, w, g_out, torch.float32, y_normalized)
    return dict(x=x, y=y, w=w, g_out=g_out, out64=out64, gx64=gx64, gy64=gy64, out32=out32, gx32=gx32, gy32=gy32)


def value_distance(got, want64):
    """Worst distance of per-image values to float64, relative to |value64|; an exact 0 must be met exactly."""
    got, want64 = got.double(), want64.double()
    zero = want64 == 0
    if bool(zero.any()) and not bool((got[zero] == 0).all()):
        return float('inf')
    rel = (got - want64).abs()[~zero] / want64.abs()[~zero]
    return float(rel.max()) if rel.numel() else 0.0


def grad_distance(got, want64):
    """Max-abs distance of a gradient to float64 over the float64 gradient's max-abs (an all-zero gradient: the max-abs itself)."""
    top = float(want64.abs().max())
    err = float((got.double() - want64).abs().max())
    return err / top if top > 0 else err


# Shapes: every register-resident channel count, one short of it and one past it, and the re-reading body at both ends;
# H x W of 1 x 1, 1 x 5, 7 x 9, 16 x 16, and flattened sizes one short of, on and one past the pixel tile, and two tiles + 3;
# B in {1, 2, 5}.  A sparse product: every C, every size and every B at least once, each tensor under 1 MB.
SHAPES = (
    (1, 1, 1, 1), (2, 2, 1, 5), (5, 3, 7, 9), (1, 63, 16, 16), (2, 64, 7, 9), (5, 64, 1, TILE + 1), (1, 64, 1, 2 * TILE + 3),
    (2, 65, 1, TILE - 1), (1, 128, 16, 16), (5, 128, 1, TILE), (2, 128, 1, 2 * TILE + 3), (2, 130, 7, 9), (1, 256, 1, TILE + 1),
    (2, 256, 16, 16), (1, 512, 1, 5), (2, 512, 1, TILE - 1), (1, 513, 1, 1), (2, 513, 1, 2 * TILE + 3), (5, 1, 16, 16), (1, 3, 1, TILE),
)
PARITY_CONTENTS = ('noise', 'near', 'scaled_small', 'scaled_large')


@functools.lru_cache(maxsize=None)
def yardsticks(content):
    """The float32 restatement's own worst distances to float64 over every parity case of the GPU file with this content,
    y_normalized on and off: (value, gradient).  The bounds are max(2 x these, FLOOR): 2 for the kernel's other summation
    order, the floor for cases the restatement gets exactly.  Nothing here comes from the code under test.
    Per content, because 'near' is the cancellation case: float32 loses three digits in xh - yh there (gradient distance
    near 1e-4 against 3e-7 for the others), and one worst over all contents would hand that slack to every case.
    C = 1 is left out and judged by uncancelled() instead: both unit vectors are 1 up to eps there, the value is an
    eps-sized remainder (1e-20) that the float32 restatement returns as 0 - a distance of 1, which would void every bound."""
    worst_v = worst_g = 0.0
    for shape in SHAPES:
        if shape[1] == 1:
            continue
        for yn in (False, True):
            c = case(content, *shape, yn)
            worst_v = max(worst_v, value_distance(c['out32'], c['out64']))
            worst_g = max(worst_g, grad_distance(c['gx32'], c['gx64']), grad_distance(c['gy32'], c['gy64']))
    return worst_v, worst_g


def bounds(content='noise'):
    v, g = yardsticks(content)
    return max(2 * v, FLOOR), max(2 * g, FLOOR)


def uncancelled(c, y_normalized=False):
    """The sizes of what cancels in a case: (value scale [B], gradient scale).  Value: mean_p sum_c w (xh^2 + yh^2).  Gradient:
    both terms of g_x (and of g_y) are at most |g| 2 w |xh - yh| / r with |xh - yh| <= 2, so max |g_out| / (H W) x 4 max w /
    min r.  Where the result is a remainder far below these (C = 1), an error is measured against them."""
    x, y, w = c['x'].double(), c['y'].double(), c['w'].double()
    xh, yh = normalize(x), (y if y_normalized else normalize(y))
    value = ((xh * xh + yh * yh) * w.view(1, -1, 1, 1)).sum(dim=1).mean(dim=(1, 2))
    r = torch.sqrt((x * x).sum(dim=1)).min() if y_normalized else torch.minimum(torch.sqrt((x * x).sum(dim=1)).min(), torch.sqrt((y * y).sum(dim=1)).min())
    hw = x.shape[2] * x.shape[3]
    return value, float(c['g_out'].abs().max()) / hw * 4 * float(w.max()) / float(r)


# --------------------------------------------------------------------------- #
# a five-tap stand-in for lpips.LPIPS(net='vgg'): .net returns five feature maps, .scaling_layer shifts and scales the
# image, .lins are the 1x1 convolutions to one channel behind an (inactive) Dropout, .L = 5
# --------------------------------------------------------------------------- #
TAP_CHANNELS = (8, 16, 24, 40, 40)


class StandInTaps(nn.Module):
    def __init__(self):
        super().__init__()
        chans = (3,) + TAP_CHANNELS
        self.convs = nn.ModuleList(nn.Conv2d(chans[i], chans[i + 1], 3, padding=1) for i in range(5))

    def forward(self, x):
        taps = []
        for i, conv in enumerate(self.convs):
            if i:
                x = nn.functional.avg_pool2d(x, 2)
            x = torch.relu(conv(x))
            taps.append(x)
        return taps


class StandInScaling(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer('shift', torch.tensor([-.030, -.088, -.188]).view(1, 3, 1, 1))
        self.register_buffer('scale', torch.tensor([.458, .448, .450]).view(1, 3, 1, 1))

    def forward(self, x):
        return (x - self.shift) / self.scale


class StandInLin(nn.Module):
    def __init__(self, channels, bias=False, out_channels=1, kernel=1):
        super().__init__()
        self.model = nn.Sequential(nn.Dropout(), nn.Conv2d(channels, out_channels, kernel, padding=kernel // 2, bias=bias))

    def forward(self, x):
        return self.model(x)


class StandInLpips(nn.Module):
    def __init__(self, seed=3):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.net, self.scaling_layer, self.L = StandInTaps(), StandInScaling(), 5
        self.lins = nn.ModuleList(StandInLin(c) for c in TAP_CHANNELS)
        with torch.no_grad():
            for p in self.net.parameters():
                p.copy_(torch.randn(p.shape, generator=gen) * (0.3 if p.dim() > 1 else 0.1))
            for lin, c in zip(self.lins, TAP_CHANNELS):
                lin.model[1].weight.copy_((0.5 + torch.rand(1, c, 1, 1, generator=gen)) / c)
            # a live first channel in every tap, as in features() above: constant 0.5 wherever the image goes
            for conv in self.net.convs:
                conv.weight[0] = 0.0
                conv.bias[0] = 0.5
        self.eval()
        self.requires_grad_(False)


def class_ref(module, in0, in1, dtype, normalize_input=False, cached=False, device='cpu'):
    """lib/metrics.py:112-137 restated for a copy of `module` (a StandInLpips) in `dtype` on `device`: [B,1].  cached: in1 is
    a tuple of normalised features.  (float32 on the GPU is the reference's own arithmetic where the class runs: the library's
    convolutions and PyTorch's elementwise head.)"""
    m = copy.deepcopy(module).to(device=device, dtype=dtype)
    feats = lambda im: m.net(m.scaling_layer((2 * im - 1) if normalize_input else im))
    f0 = feats(in0.to(device=device, dtype=dtype))
    f1 = [t.to(device=device, dtype=dtype) for t in in1] if cached else feats(in1.to(device=device, dtype=dtype))
    return sum(head_ref(a, b, lin.model[1].weight.reshape(-1), dtype, y_normalized=cached).unsqueeze(1)
               for a, b, lin in zip(f0, f1, m.lins))


def class_features_ref(module, im, dtype, normalize_input=False, device='cpu'):
    """What lib/metrics.py:112-123 returns for in1=None, restated for a copy of `module` in `dtype` on `device`: the
    normalised features of the first L taps, in order, of net(scaling_layer(im)) - after 2 im - 1 with normalize_input."""
    m = copy.deepcopy(module).to(device=device, dtype=dtype)
    im = im.to(device=device, dtype=dtype)
    taps = m.net(m.scaling_layer((2 * im - 1) if normalize_input else im))
    return tuple(normalize(taps[i]) for i in range(m.L))


def features_ref(weights, f0, f1, y_normalized=False):
    """The distance [B] of given feature maps in float64, and its gradients to every map of f0 for a cotangent of ones."""
    leaves = [f.double().requires_grad_() for f in f0]
    out = sum(head_ref(a, b.double(), w.double(), torch.float64, y_normalized) for a, b, w in zip(leaves, f1, weights))
    return out.detach(), torch.autograd.grad(out.sum(), leaves)
