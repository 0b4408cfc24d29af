"""The LPIPS distance head (metrics.lpips_distance; csrc/nfi_lpips.inc) against the PyTorch expression of lib/metrics.py:104-133
under PyTorch-ROCm on the same GPU:
    python tools/lpips_head_bench.py [--calls 50] [--warmup 5] [--out times.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/lpips_head_bench.py --trace hip     (or: reference)

What is timed: everything the reference's LPIPSLoss does AFTER the VGG network, for the five VGG16 taps of a 128 x 128 image
([.,64,128,128], [.,128,64,64], [.,256,32,32], [.,512,16,16], [.,512,8,8]), at 64 image pairs (the loss of run.py:2232 at
BASELINE cfg3's per-GPU shape: 4 images x (1 + 15 augmentations)) and at 4 (the monitor call of run.py:2249): forward alone
(no gradient), and forward + backward to the prediction's features.  The network itself is not run: RANDOM features
(relu(randn), the target a ReLU'd perturbation of the prediction) stand in for VGG's, because neither the lpips package nor
its weights are on the machine; the head's time does not depend on the values.  The comparator restates the reference's
formulas in torch - normalize_tensor with eps added to the norm, the lin layers as conv2d with a [1,C,1,1] weight - and
imports nothing of the reference.

Method: device events around each call on the launch stream, `--warmup` rounds first, then `--calls` timed rounds in which
the two implementations alternate within this one process; per figure the median, the 10th and 90th percentile.  Also each
implementation's distance to the float64 restatement at 4 pairs (on the CPU; at 64 pairs float64 on the CPU is 2 GB of
features and minutes, so it is left out and said so).

--trace hip | reference: a run of its own for the profiler, no timing: the named implementation alone makes 10 calls per
case and nothing else touches the device, so the kernel trace's call counts divide by 10 x 4 = 40 into launches per call."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from nerf_from_image_amd import metrics  # noqa: E402

TAPS = ((64, 128), (128, 64), (256, 32), (512, 16), (512, 8))       # (channels, side) of the VGG16 taps at 128 x 128
PAIRS = (64, 4)
TRACE_CALLS = 10
EPS = 1e-10


def normalize(x):
    return x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + EPS)


def reference_distance(f0, f1, weights):
    """lib/metrics.py:104-110, 130-133 restated: [B,1]."""
    return sum(F.conv2d((normalize(x) - normalize(y)).square(), w.view(1, -1, 1, 1)).mean(dim=[2, 3]) for x, y, w in zip(f0, f1, weights))


def make_features(pairs, dev, g):
    f0, f1, weights = [], [], []
    for c, side in TAPS:
        x = torch.relu(torch.randn(pairs, c, side, side, device=dev, generator=g))
        x[:, 0] += 0.5
        y = torch.relu(x + 0.5 * torch.randn(pairs, c, side, side, device=dev, generator=g))
        y[:, 0] += 0.25
        f0.append(x); f1.append(y)
        weights.append((torch.rand(c, device=dev, generator=g) + 0.5) / c)
    return f0, f1, weights


def alternate(fns, n, warm):
    """Per function the sorted device-event times (ms) of n calls, the functions called in turn, after `warm` rounds."""
    for _ in range(warm):
        for f in fns:
            f()
    torch.cuda.synchronize()
    events = [[] for _ in fns]
    for _ in range(n):
        for j, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); f(); b.record()
            events[j].append((a, b))
    torch.cuda.synchronize()
    return [sorted(a.elapsed_time(b) for a, b in ev) for ev in events]


def spread(ts):
    n = len(ts)
    return dict(median_ms=ts[n // 2], p10_ms=ts[n // 10], p90_ms=ts[(9 * n) // 10])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--trace', choices=('hip', 'reference'), default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(0)
    records, slower = [], []
    for pairs in PAIRS:
        f0, f1, weights = make_features(pairs, dev, g)
        feature_bytes = 2 * 4 * sum(t.numel() for t in f0)
        leaves = [t.clone().requires_grad_() for t in f0]

        def forward(fn):
            with torch.no_grad():
                return fn(f0, f1, weights)

        def forward_backward(fn):
            out = fn(leaves, f1, weights)
            return out, torch.autograd.grad(out.sum(), leaves)

        for mode, run in (('forward', forward), ('forward+backward', forward_backward)):
            hip = lambda: run(metrics.lpips_distance)
            ref = lambda: run(reference_distance)
            if a.trace:
                for _ in range(TRACE_CALLS):
                    (hip if a.trace == 'hip' else ref)()
                torch.cuda.synchronize()
                print('trace: %d calls of %s, %s at %d pairs' % (TRACE_CALLS, a.trace, mode, pairs), flush=True)
                continue
            t_hip, t_ref = alternate([hip, ref], a.calls, a.warmup)
            rec = dict(pairs=pairs, mode=mode, calls=a.calls, feature_megabytes=feature_bytes / 1e6, hip=spread(t_hip), reference=spread(t_ref),
                       ratio=t_ref[len(t_ref) // 2] / t_hip[len(t_hip) // 2])
            got_hip, got_ref = hip(), ref()
            if mode == 'forward':
                rec['hip_vs_reference'] = float(((got_hip - got_ref).abs() / got_ref.abs()).max())
            else:
                rec['hip_vs_reference'] = max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(got_hip[1], got_ref[1]))
            if pairs <= 4:                  # float64 on the CPU
                l64 = [t.detach().cpu().double().requires_grad_() for t in f0]
                out64 = reference_distance(l64, [t.cpu().double() for t in f1], [w.cpu().double() for w in weights])
                if mode == 'forward':
                    dist = lambda got: float(((got.cpu().double() - out64.detach()).abs() / out64.detach().abs()).max())
                    rec['hip_error'], rec['reference_error'] = dist(got_hip), dist(got_ref)
                else:
                    g64 = torch.autograd.grad(out64.sum(), l64)
                    dist = lambda got: max(float((p.cpu().double() - q).abs().max() / q.abs().max()) for p, q in zip(got[1], g64))
                    rec['hip_error'], rec['reference_error'] = dist(got_hip), dist(got_ref)
            records.append(rec)
            if rec['ratio'] < 1.0:
                slower.append((pairs, mode))
            print('lpips head, %2d pairs, %-16s (%.0f MB of features): HIP %.4f ms (p10 %.4f, p90 %.4f), reference %.4f ms (p10 %.4f, p90 %.4f), '
                  'ratio %.2f; HIP against reference %.2e; distance to float64: %s' % (
                      pairs, mode, rec['feature_megabytes'], rec['hip']['median_ms'], rec['hip']['p10_ms'], rec['hip']['p90_ms'],
                      rec['reference']['median_ms'], rec['reference']['p10_ms'], rec['reference']['p90_ms'], rec['ratio'], rec['hip_vs_reference'],
                      'HIP %.2e, reference %.2e' % (rec['hip_error'], rec['reference_error']) if 'hip_error' in rec else 'not computed at this size'),
                  flush=True)
        del f0, f1, leaves
        torch.cuda.empty_cache()
    if a.trace:
        return
    print('HIP slower than the reference at: %s' % (slower or 'no size and mode'))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(dict(device=torch.cuda.get_device_name(0), taps=TAPS, records=records, slower=slower), open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
