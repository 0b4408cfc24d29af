"""The head of a synthesis layer restated in plain torch from the reference's own expressions, runnable in a given dtype, and
the seeded inputs of tests/test_synth_head_abi.py and tests/test_synth_head_gpu.py.  float64 is the yardstick; its gradients
are autograd's.

    styles = (latent @ (A * weight_gain).T + bias * bias_gain) * style_gain                         (stylegan.py:173-177, 373)
    dcoefs = ((W[None] * styles[:, None, :, None, None]).square().sum([2, 3, 4]) + 1e-8).rsqrt()    (stylegan.py:127-130)
    out    = x * styles[:, :, None, None]                                                           (stylegan.py:132)

The demodulation is restated as the reference writes it - the [B,O,I,kh,kw] product - not in the factored form the kernels
use (`dcoefs_factored` is that form; test_synth_head_abi.py checks the two agree in float64).

Also here: the small-network recipe of tests/test_synth_tail_gpu.py (copied, not imported: that is a test file) with its
rule for comparing a fused network with the unfused one."""
import copy
import functools

import torch

FLOOR = 2.0 ** -21                          # the tail tests' floor (tests/synth_tail_util.py), here times max(1, max |want|)

# (B, D, I, O, K, demodulate, style_gain)
HEAD_SHAPES = {
    'one': (1, 1, 1, 1, 1, True, 1.0),
    'wave_and_tail': (2, 70, 5, 3, 9, True, 1.0),              # D: one wave plus a tail of 6
    'odd_row': (3, 130, 33, 16, 9, True, 1.0),                 # I K = 297, not a multiple of 64
    'torgb': (2, 32, 64, 96, 1, False, 0.125),                 # OutputLayer: no demodulation, style_gain = 1 / sqrt(64)
    'largest': (4, 512, 512, 512, 9, True, 1.0),               # the real largest layer
    'ten_images': (10, 40, 70, 19, 9, True, 1.0),              # two groups of 8 images; 19 rows = 3 chunks of 8 in the backward
    'generic_taps': (2, 20, 300, 7, 4, True, 1.0),             # K neither 1 nor 9; I spans two blocks of 256 threads
}


def head_ref(latent, A, a_bias, weight_gain, bias_gain, W, demodulate=True, style_gain=1.0, dtype=torch.float64):
    """(styles, dcoefs or None) in `dtype`, written as the reference writes them (inputs are cast; gains are Python floats)."""
    cast = (lambda t: None if t is None else t.to(dtype))
    latent, A, a_bias, W = cast(latent), cast(A), cast(a_bias), cast(W)
    weight = A * weight_gain
    b = a_bias * bias_gain if a_bias is not None else None
    styles = torch.nn.functional.linear(latent, weight, b)
    if style_gain != 1.0:
        styles = styles * style_gain
    if not demodulate:
        return styles, None
    bs = latent.shape[0]
    w = W.reshape(W.shape[0], W.shape[1], -1, 1).unsqueeze(0)
    w = w * styles.reshape(bs, 1, -1, 1, 1)
    return styles, (w.square().sum(dim=[2, 3, 4]) + 1e-8).rsqrt()


def dcoefs_factored(styles, W):
    """rsqrt(sum_i styles^2 Q[o,i] + 1e-8), Q[o,i] = sum_k W[o,i,k]^2: the form the kernels evaluate."""
    Q = W.reshape(W.shape[0], W.shape[1], -1).square().sum(dim=2)
    return (styles.square() @ Q.T + 1e-8).rsqrt()


def modulate_ref(x, styles, dtype=torch.float64):
    x, styles = x.to(dtype), styles.to(dtype)
    return x * styles.reshape(styles.shape + (1,) * (x.dim() - 2))


def tolerance(e32, want):
    """max(2 x e32, 2^-21 x max(1, max |want|)): e32 is the float32 restatement's own worst distance to float64."""
    return max(2.0 * e32, FLOOR * max(1.0, float(want.abs().max())))


def make_head_inputs(B, D, I, O, K, bias=True, zero=False, seed=1):
    g = torch.Generator().manual_seed(7919 * seed + 131 * D + 17 * I + 3 * O + K + B)
    kh = 3 if K == 9 else (2 if K == 4 else 1)
    t = dict(latent=torch.randn(B, D, generator=g), A=torch.randn(I, D, generator=g),
             a_bias=(1.0 + 0.5 * torch.randn(I, generator=g)) if bias else None, W=torch.randn(O, I, kh, K // kh, generator=g),
             g_styles=torch.randn(B, I, generator=g), g_dcoefs=torch.randn(B, O, generator=g))
    if zero:
        t['latent'].zero_()
        if bias:
            t['a_bias'].zero_()
    t['weight_gain'], t['bias_gain'] = 1.0 / D ** 0.5, 1.0
    return t


HEAD_GRADS = ('g_latent', 'g_affine_weight', 'g_affine_bias', 'g_weight')


def _run_head(t, demodulate, style_gain, dtype):
    names = [n for n in ('latent', 'A', 'a_bias', 'W') if t[n] is not None]
    leaves = {n: t[n].detach().clone().to(dtype).requires_grad_() for n in names}
    styles, dcoefs = head_ref(leaves['latent'], leaves['A'], leaves.get('a_bias'), t['weight_gain'], t['bias_gain'], leaves['W'], demodulate,
                              style_gain, dtype)
    target = (styles * t['g_styles'].to(dtype)).sum()
    if demodulate:
        target = target + (dcoefs * t['g_dcoefs'].to(dtype)).sum()
    grads = torch.autograd.grad(target, [leaves[n] for n in names], allow_unused=True)
    out = dict(zip(names, grads))
    res = {'styles': styles.detach(), 'g_latent': out['latent'], 'g_affine_weight': out['A']}
    if demodulate:
        res['dcoefs'] = dcoefs.detach()
        res['g_weight'] = out['W'].reshape(out['W'].shape[0], out['W'].shape[1], -1)
    if 'a_bias' in out:
        res['g_affine_bias'] = out['a_bias']
    return res


@functools.lru_cache(maxsize=None)
def head_case(B, D, I, O, K, demodulate=True, style_gain=1.0, bias=True, zero=False):
    """Everything the tests need of one head case, computed once on the CPU: the inputs (with the two upstream gradients), the
    float64 yardstick - styles, dcoefs and the gradients of sum(styles g_styles) + sum(dcoefs g_dcoefs) with respect to the
    latent, the affine weight and bias and the convolution weight - and e32, the float32 restatement's own worst distance to
    it, per quantity."""
    t = make_head_inputs(B, D, I, O, K, bias, zero)
    want = _run_head(t, demodulate, style_gain, torch.float64)
    own = _run_head(t, demodulate, style_gain, torch.float32)
    e32 = {k: float((own[k].double() - want[k]).abs().max()) for k in want}
    return dict(inputs=t, want=want, e32=e32, demodulate=demodulate, style_gain=style_gain)


@functools.lru_cache(maxsize=None)
def modulate_case(B, C, n, seed=1):
    """x [B,C,n], styles [B,C], g_out [B,C,n]; the yardstick out, g_x, g_styles and e32 per quantity."""
    g = torch.Generator().manual_seed(104729 * seed + 31 * n + 7 * C + B)
    t = dict(x=torch.randn(B, C, n, generator=g), styles=torch.randn(B, C, generator=g), g_out=torch.randn(B, C, n, generator=g))

    def run(dtype):
        x, s = t['x'].to(dtype).requires_grad_(), t['styles'].to(dtype).requires_grad_()
        out = modulate_ref(x, s, dtype)
        g_x, g_s = torch.autograd.grad(out, (x, s), t['g_out'].to(dtype))
        return {'out': out.detach(), 'g_x': g_x, 'g_styles': g_s}
    want, own = run(torch.float64), run(torch.float32)
    return dict(inputs=t, want=want, e32={k: float((own[k].double() - want[k]).abs().max()) for k in want})


# ---------------------------------------------------------------------------------------------------------------------
# the real SynthesisNetwork: tests/test_synth_tail_gpu.py's recipe and rule
# ---------------------------------------------------------------------------------------------------------------------
class drawn_noise:
    """torch.randn served from a CPU generator for the duration of the block, so that the float64 yardstick on the CPU and
    the float32 runs on the GPU see the same noise images (the device generators differ)."""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def __enter__(self):
        self.real = torch.randn
        real, g = self.real, self.g
        torch.randn = lambda size, device=None, **kw: real(size, generator=g, **kw).to(device)
        return self

    def __exit__(self, *exc):
        torch.randn = self.real
        return False


# A tensor with fewer elements has no worst case of its own (test_synth_tail_gpu.py): its bound is no smaller than
# 2 x e32 x max |T64|, e32 the unfused network's worst relative distance over the tensors that are large enough
FEW = 32
# float32 rounding through the network relative to a tensor's largest magnitude (derived in test_synth_tail_gpu.py)
E32_NETWORK = 2.0 ** -16


def small_network(stylegan, seed=0):
    torch.manual_seed(seed)
    net = stylegan.SynthesisNetwork(w_dim=32, img_resolution=16, img_channels=96, channel_max=16)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith('noise_strength'):
                p.fill_(0.3)
            elif name.endswith('bias'):
                p.normal_()
    g = torch.Generator().manual_seed(seed + 1)
    return net, torch.randn(2, net.num_ws, 32, generator=g), torch.randn(2, 96, 16, 16, generator=g)


def network_step(net, ws, weight, noise_mode, training, noise_seed=7):
    """(planes, {name: gradient}) of sum(planes * weight), with respect to ws and every parameter."""
    net.train(training)
    ws = ws.clone().requires_grad_()
    with drawn_noise(noise_seed):
        planes = net(ws, noise_mode=noise_mode)
    names, params = zip(*net.named_parameters())
    grads = torch.autograd.grad((planes * weight).sum(), (ws,) + params, allow_unused=True)
    return planes.detach(), dict(zip(('ws',) + names, grads))


_YARDSTICKS = {}


def network_yardstick(stylegan, noise_mode, training):
    key = (noise_mode, training)
    if key not in _YARDSTICKS:
        net, ws, weight = small_network(stylegan)
        _YARDSTICKS[key] = network_step(copy.deepcopy(net).double(), ws.double(), weight.double(), noise_mode, training)
    return _YARDSTICKS[key]


def network_distances(run, yardstick):
    """{name: (worst distance to the float64 yardstick, the yardstick's largest magnitude, elements)}"""
    planes64, grads64 = yardstick
    out = {'planes': (float((run[0].cpu().double() - planes64).abs().max()), float(planes64.abs().max()), planes64.numel())}
    for k, g64 in grads64.items():
        assert (g64 is None) == (run[1][k] is None), k
        if g64 is not None:
            out[k] = (float((run[1][k].cpu().double() - g64).abs().max()), float(g64.abs().max()), g64.numel())
    return out


def network_rule(own, got):
    """The tail test's rule: a tensor T of the fused run is within max(2 x the unfused run's own distance, 2^-21) of the
    yardstick; below FEW elements the bound is no smaller than 2 x e32 x max |T64|.  Returns (missed, worst, e32)."""
    e32 = max(err / scale for err, scale, n in own.values() if scale > 0 and n >= FEW)
    worst, missed = (0.0, None), []
    for k, (err, scale, n) in got.items():
        tol = max(2 * own[k][0], FLOOR)
        if n < FEW:
            tol = max(tol, 2 * e32 * scale)
        if err > tol:
            missed.append((k, n, err, tol))
        worst = max(worst, (err / tol, k))
    return missed, worst, e32
