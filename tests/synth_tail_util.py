"""The tail of a synthesis layer restated in plain torch from its formula, runnable in a given dtype, and the seeded inputs
of tests/test_synth_tail_abi.py and tests/test_synth_tail_gpu.py.  float64 is the yardstick.

    f   = up ? sum_{a,b in 0..3} (4 taps[a][b]) y[i + a - 1, j + b - 1]   (zero outside y)  :  y
    out = lrelu_slope(((noise + f * dcoefs[b,c]) + bias[c]) * act_gain)                      (no lrelu when activate is off)

`variant` breaks the restatement on purpose (test_synth_tail_abi checks that the parity bound tells each from the truth)."""
import functools
import math

import torch
import torch.nn.functional as F

FLOOR = 2.0 ** -21                          # tests/test_blur_gpu.py's FLOOR: four units in the last place of 1.0
KINK = 1e-3                                 # |pre64| < KINK * std(pre64): a float32 pre-activation may sit across the kink
VARIANTS = ('shifted', 'no_padding', 'no_gain', 'no_noise', 'wrong_side')
ACT_GAIN = math.sqrt(2.0)


def bilinear_taps():
    h = torch.tensor([1.0, 3.0, 3.0, 1.0])
    h = h[:, None] * h[None, :]
    return h / h.sum()


def asymmetric_taps():
    """16 different values, not an outer product, no symmetry: a flipped, transposed or separable reading shows."""
    a, b = torch.arange(4.0).view(4, 1), torch.arange(4.0).view(1, 4)
    t = 1.0 + 4.0 * a + b + 0.37 * ((7.0 * a + 3.0 * b) % 5.0) - 2.5 * (a == b)
    return (t / t.abs().sum()).float()


TAPS = {'bilinear': bilinear_taps, 'asymmetric': asymmetric_taps}


def up_filter(y, taps, gain=4.0, variant=None):
    """y [B,C,R+1,R+1] -> [B,C,R,R]: sum_{a,b} (gain taps[a][b]) y[i + a - 1, j + b - 1], zero outside y."""
    R = y.shape[-1] - 1
    if variant == 'no_gain':
        gain = 1.0
    yp = F.pad(y, (1, 1, 1, 1), mode='replicate') if variant == 'no_padding' else F.pad(y, (1, 1, 1, 1))
    if variant == 'shifted':
        yp = torch.roll(yp, 1, dims=-1)
    f = torch.zeros(y.shape[:2] + (R, R), dtype=y.dtype)
    for a in range(4):
        for b in range(4):
            f = f + (gain * taps[a, b]) * yp[..., a:a + R, b:b + R]
    return f


def tail_ref(y, dcoefs, noise, bias, taps, act_gain, up, activate=True, slope=0.2, dtype=torch.float64, variant=None,
             return_pre=False):
    """The tail in `dtype` (inputs are cast).  noise: None, [B,1,R,R] or [R,R]."""
    cast = (lambda t: None if t is None else t.to(dtype))
    y, dcoefs, noise, bias = cast(y), cast(dcoefs), cast(noise), cast(bias)
    f = up_filter(y, taps.to(dtype), variant=variant) if up else y
    x = f * dcoefs[:, :, None, None]
    if noise is not None and variant != 'no_noise':
        x = noise + x
    x = x + bias[None, :, None, None]
    pre = x * act_gain
    if not activate:
        out = pre
    elif variant == 'wrong_side':
        out = torch.where(pre > 0, pre * slope, pre)
    else:
        out = torch.where(pre > 0, pre, pre * slope)
    return (out, pre) if return_pre else out


IMPULSES = ('corner', 'edge', 'interior')


def impulse_at(place, n):
    return {'corner': (0, 0), 'edge': (n - 1, n // 2), 'interior': (n // 2, max(n // 2 - 1, 0))}[place]


def make_inputs(B, C, R, up, noise_kind, taps_kind='bilinear', content='noise', seed=1):
    """CPU float32 inputs of one case.  noise_kind: None, 'batch' ([B,1,R,R]) or 'shared' ([R,R]); content: 'noise'
    (unit normal) or 'impulse_<place>' (y is one 1.0 per plane on zeros).  The seed is one with which no case of the two
    test files has more than 0.5 % of its elements near the kink (a single element is 25 % of the smallest case; the
    tests assert the share)."""
    g = torch.Generator().manual_seed(1000 * seed + 97 * R + 13 * B + C + (5 if up else 0))
    n = R + 1 if up else R
    if content == 'noise':
        y = torch.randn(B, C, n, n, generator=g)
    else:
        y = torch.zeros(B, C, n, n)
        iy, ix = impulse_at(content[len('impulse_'):], n)
        y[:, :, iy, ix] = 1.0
    t = dict(y=y, dcoefs=torch.randn(B, C, generator=g), bias=torch.randn(C, generator=g), g_out=torch.randn(B, C, R, R, generator=g),
             taps=TAPS[taps_kind](), noise=None)
    if noise_kind == 'batch':
        t['noise'] = torch.randn(B, 1, R, R, generator=g)
    elif noise_kind == 'shared':
        t['noise'] = torch.randn(R, R, generator=g)
    return t


GRADS = ('g_y', 'g_dcoefs', 'g_bias', 'g_noise')


def _run(t, up, activate, dtype, g_out):
    leaves = {k: t[k].detach().clone().to(dtype).requires_grad_() for k in ('y', 'dcoefs', 'bias', 'noise') if t[k] is not None}
    out = tail_ref(leaves['y'], leaves['dcoefs'], leaves.get('noise'), leaves['bias'], t['taps'], ACT_GAIN if activate else 1.0, up,
                   activate, dtype=dtype)
    names = [k for k in ('y', 'dcoefs', 'bias', 'noise') if k in leaves]
    grads = torch.autograd.grad(out, [leaves[k] for k in names], g_out.to(dtype))
    return out.detach(), {'g_' + k: v for k, v in zip(names, grads)}


@functools.lru_cache(maxsize=None)
def case(B, C, R, up, noise_kind, activate, taps_kind='bilinear', content='noise'):
    """Everything the tests need of one case, computed once on the CPU: the inputs, the masked upstream gradient, the float64
    yardstick (out and the four gradients), and e32 - the float32 restatement's own worst distance to it - per quantity.
    The upstream gradient is zero where |pre64| < KINK * std(pre64): those elements drop out of every sum on both sides."""
    t = make_inputs(B, C, R, up, noise_kind, taps_kind, content)
    gain = ACT_GAIN if activate else 1.0
    _, pre = tail_ref(t['y'], t['dcoefs'], t['noise'], t['bias'], t['taps'], gain, up, activate, return_pre=True)
    if activate:
        std = float(pre.std()) if pre.numel() > 1 else float(pre.abs().max())
        near = pre.abs() < KINK * std
    else:
        near = torch.zeros_like(pre, dtype=torch.bool)
    g_out = torch.where(near, torch.zeros(()), t['g_out'])
    out64, grads64 = _run(t, up, activate, torch.float64, g_out)
    out32, grads32 = _run(t, up, activate, torch.float32, g_out)
    e32 = {'out': float((out32.double() - out64).abs().max())}
    for k in grads64:
        e32[k] = float((grads32[k].double() - grads64[k]).abs().max())
    return dict(inputs=t, gain=gain, g_out=g_out, near=near, excluded=float(near.float().mean()), out=out64, grads=grads64, e32=e32)


def tolerance(e32):
    return max(2.0 * e32, FLOOR)
