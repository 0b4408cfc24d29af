"""Timing of the view-direction mapper's per-ray trunk (models/generator.py:223-239): the PyTorch modules against the HIP
node (generator.hip_ray_feature), forward and forward + backward, at N = 1 x 64^2, 1 x 128^2 and 8 x 128^2 rays.

    python tools/viewdir_mapper_bench.py [--rounds 7] [--reps 20] [--out FILE]

Protocol: HIP events on the launch stream around `reps` back-to-back calls (no host synchronise inside the window), after a
warm-up of every shape and both sides; `rounds` such windows per side, the two sides ALTERNATING round by round; reported
per shape and side: median, minimum and maximum over the rounds of the window's time per call (ms).  forward + backward is
one forward under autograd and one backward of a random upstream gradient, gradients to the 18 parameters and to the
view directions (fwd_bwd_directions_only: to the view directions alone - on the PyTorch side autograd then skips the
weight gradients, on the HIP side the node calls the backward without parameter-gradient pointers).  The module is a stand-alone copy of the trunk with the reference's arithmetic (EqualizedLinear gains,
LayerNorm, joins); the two sides are compared on the timed inputs first: the output by its largest difference relative to
its largest entry (asserted), two gradients by relative L2 (reported only - among thousands of random rays a few put a
LeakyReLU input within fp32 rounding of zero, and the two fp32 forwards may then take different slopes for that ray).
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import nerf_from_image_amd.generator as nfi_gen  # noqa: E402

SHAPES = (('1x64^2', (1, 64, 64)), ('1x128^2', (1, 128, 128)), ('8x128^2', (8, 128, 128)))


class _EqLinear(nn.Module):
    def __init__(self, i, o, bias=True):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(o, i))
        self.bias = nn.Parameter(0.3 * torch.randn(o)) if bias else None
        self.gain = 1.0 / math.sqrt(i)

    def forward(self, x):
        return F.linear(x, self.weight * self.gain, self.bias)


class Trunk(nn.Module):
    """fc0 .. fc6 / norm1 .. norm4 as the class runs them, op for op (in-place activations and joins included)."""

    def __init__(self):
        super().__init__()
        self.fc0 = _EqLinear(3, 64)
        for i in range(1, 5):
            setattr(self, 'fc%d' % i, _EqLinear(64, 64, bias=False))
            setattr(self, 'norm%d' % i, nn.LayerNorm(64))
        self.fc5, self.fc6 = _EqLinear(64, 64), _EqLinear(64, 32)
        self.output = _EqLinear(32, 10)          # (the closure's layer: what makes the module mapper-shaped; not timed)
        self.relu = nn.LeakyReLU(0.2, inplace=True)
        with torch.no_grad():
            for i in range(1, 5):
                n = getattr(self, 'norm%d' % i)
                n.weight.add_(0.3 * torch.randn(64))
                n.bias.add_(0.2 * torch.randn(64))

    def forward(self, v):
        scale = math.sqrt(2) / 2
        x = self.relu(self.fc0(v))
        s = x
        x = self.relu(self.norm1(self.fc1(x)))
        x = self.relu(self.norm2(self.fc2(x)))
        x = (x + s).mul_(scale)
        s = x
        x = self.relu(self.norm3(self.fc3(x)))
        x = self.relu(self.norm4(self.fc4(x)))
        x = (x + s).mul_(scale)
        return self.fc6(self.relu(self.fc5(x)))


def window(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def spread(v):
    v = sorted(v)
    return {'median_ms': round(v[len(v) // 2], 4), 'min_ms': round(v[0], 4), 'max_ms': round(v[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('viewdir_mapper_bench: needs a GPU (a CPU run measures nothing)')
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    trunk = Trunk().to(dev)
    import copy
    frozen = copy.deepcopy(trunk).requires_grad_(False)
    result = {'tool': 'viewdir_mapper_bench', 'device': torch.cuda.get_device_name(0), 'rounds': a.rounds, 'reps_per_window': a.reps,
              'unit': 'ms per call, HIP events around a window of back-to-back calls', 'shapes': {}}
    for name, (b, h, w) in SHAPES:
        v = torch.randn(b, h, w, 1, 3, device=dev)
        v = (v / v.norm(dim=-1, keepdim=True)).requires_grad_()
        g = torch.randn(b, h, w, 1, 32, device=dev)
        leaves = [v] + list(nfi_gen.viewdir_mapper_parameters(trunk))

        def fwd(side):
            with torch.no_grad():
                return trunk(v) if side == 'torch' else nfi_gen.hip_ray_feature(trunk, v)

        def fwd_bwd(side):
            x = trunk(v) if side == 'torch' else nfi_gen.hip_ray_feature(trunk, v)
            return torch.autograd.grad(x, leaves, g)

        def fwd_bwd_frozen(side):                  # the inversion loop: parameters frozen, only the directions differentiated
            x = trunk(v) if side == 'torch' else nfi_gen.hip_ray_feature(frozen, v)
            return torch.autograd.grad(x, [v], g)
        # the two sides compute the same thing on the timed inputs
        x_t, x_h = fwd('torch'), fwd('hip')
        g_t, g_h = fwd_bwd('torch'), fwd_bwd('hip')
        l2 = (lambda p, q: float((p - q).norm() / q.norm()))
        agree = {'feature_max': float((x_h - x_t).abs().max() / x_t.abs().max()), 'g_viewdir_l2': l2(g_h[0], g_t[0]),
                 'g_fc3_w_l2': l2(g_h[9], g_t[9])}
        assert agree['feature_max'] < 1e-5, agree
        cases = {'fwd': fwd, 'fwd_bwd': fwd_bwd, 'fwd_bwd_directions_only': fwd_bwd_frozen}
        times = {k: {'torch': [], 'hip': []} for k in cases}
        for k, fn in cases.items():
            for side in ('torch', 'hip'):             # warm-up
                window(lambda: fn(side), 3)
            for _ in range(a.rounds):
                for side in ('torch', 'hip'):
                    times[k][side].append(window(lambda: fn(side), a.reps))
        rep = {'rays': b * h * w, 'agreement': {k: float('%.2e' % e) for k, e in agree.items()}}
        for k in cases:
            rep[k] = {side: spread(times[k][side]) for side in ('torch', 'hip')}
            rep[k]['speedup_of_medians'] = round(rep[k]['torch']['median_ms'] / rep[k]['hip']['median_ms'], 2)
        result['shapes'][name] = rep
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
