"""The tail of a synthesis layer as one HIP node (synthesis.layer_tail; csrc/nfi_synth_tail.inc) against the same expression in
PyTorch-ROCm on the same GPU, and the end-to-end legs of tools/end_to_end.py with and without attach(fused_synthesis_tail=True):
    python tools/bench_synth_tail.py [--windows 9] [--window-ms 30] [--out times.json]
    python tools/bench_synth_tail.py --e2e [--iters 12] [--rounds 2] [--batches 4 1] [--out e2e.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \\
        python tools/bench_synth_tail.py --leg inversion [--fused] --markers --sidecar side.json        (then tools/phase_split.py DIR side.json)

What is timed (default mode): everything SynthesisLayer.forward (models/stylegan.py:325-356) does after its convolution, at
the shapes the real network has - [B,512,R,R] for R = 8 .. 64, [B,256,128,128], [B,128,256,256], each as an `up` layer (the
input is the transposed convolution's [B,C,R+1,R+1]) and as a plain one, at B = 8 and B = 1, with a [B,1,R,R] noise image:
forward alone (no gradient), and forward + backward to y, dcoefs, bias and the noise (a training step: noise_strength is a
parameter).  The comparator restates stylegan.py:58-69, 101-105, 139-140, 351-355 in torch - the 4x4 filter as F.conv2d on
[B*C,1,.,.], addcmul, + bias, mul_, leaky_relu in place - and imports nothing of the reference.

Method: a timed window is one pair of device events around K back-to-back calls, K chosen per shape and mode so that a window
lasts about `--window-ms` (one event pair per call would time, at the small shapes, the gap the queue runs dry in rather
than the calls: a call there is 15 - 300 us, bound by the host's enqueue).  `--prewarm-s` seconds of untimed calls at the
start of the process, one warm-up window each per shape and mode, then `--windows` timed
windows in which the two implementations alternate within this one process; a figure is a window's time / K, reported as
the median, the 10th and the 90th percentile over the windows.  A shape counts as `slower` when the node's median exceeds
the PyTorch median by more than the wider of the two p10 .. p90 spreads.  The buffers are the same in every call: whatever
fits the 256 MB infinity cache (everything but [8,256,128,128] and [8,128,256,256]) is served from it on both sides, so
the small shapes compare launch counts and enqueue cost, not HBM traffic.

--e2e: tools/end_to_end.py's inversion and generator-step legs (its own scenes, steps and timing) on attach()'s model and on
a model attached with attach(fused_synthesis_tail=True) (the legs' own keyword), `--rounds` times each, alternating, at the
legs' 4 images and at 1, where a step is bound by launches.  --leg: one such leg alone, for the profiler, writing the
sidecar tools/phase_split.py reads."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from nerf_from_image_amd import synthesis  # noqa: E402

SHAPES = ((512, 8), (512, 16), (512, 32), (512, 64), (256, 128), (128, 256))        # (channels, R) of the synthesis layers
BATCHES = (8, 1)
GAIN, SLOPE = 2.0 ** 0.5, 0.2


def torch_tail(y, dcoefs, noise, bias, taps, up):
    """stylegan.py:58-69 + 101-105 (filter2d, gain 4), 139-140, 351-355 restated."""
    b, c = y.shape[:2]
    x = y
    if up:
        x = F.conv2d(y.flatten(0, 1).unsqueeze(1), (taps * 4)[None, None], padding=1)
        x = x.view(b, c, x.shape[2], x.shape[3])
    x = torch.addcmul(noise, x, dcoefs.reshape(b, -1, 1, 1))
    x = x + bias.view(1, -1, 1, 1)
    x = x.mul_(GAIN)
    return F.leaky_relu(x, SLOPE, inplace=True)


def hip_tail(y, dcoefs, noise, bias, taps, up):
    return synthesis.layer_tail(y, dcoefs, noise, bias, taps, GAIN, up, True, SLOPE)


def alternate(fns, windows, window_ms):
    """Per function the sorted per-call device times (ms) of `windows` windows of K calls each, the functions taking turns
    window by window after one warm-up window each; K makes a window last about window_ms.  Returns (times, [K per function])."""
    def window(f, k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(k):
            f()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / k
    ks = []
    for f in fns:
        for _ in range(3):
            f()
        ks.append(max(4, min(2000, int(window_ms / max(window(f, 4), 1e-3)))))
        window(f, ks[-1])
    times = [[] for _ in fns]
    for _ in range(windows):
        for j, f in enumerate(fns):
            times[j].append(window(f, ks[j]))
    return [sorted(t) for t in times], ks


def spread(ts):
    n = len(ts)
    return dict(median_ms=ts[n // 2], p10_ms=ts[n // 10], p90_ms=ts[(9 * n) // 10])


def micro(a):
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(0)
    taps = torch.tensor([1.0, 3.0, 3.0, 1.0], device=dev)
    taps = taps[:, None] * taps[None, :]
    taps = taps / taps.sum()
    records, slower = [], []
    for batch in BATCHES:
        for c, r in SHAPES:
            for up in (True, False):
                n = r + 1 if up else r
                y = torch.randn(batch, c, n, n, device=dev, generator=g)
                dcoefs = torch.rand(batch, c, device=dev, generator=g) + 0.5
                noise = torch.randn(batch, 1, r, r, device=dev, generator=g)
                bias = torch.randn(c, device=dev, generator=g)
                g_out = torch.randn(batch, c, r, r, device=dev, generator=g)
                leaves = [t.clone().requires_grad_() for t in (y, dcoefs, noise, bias)]

                def forward(fn):
                    with torch.no_grad():
                        return fn(y, dcoefs, noise, bias, taps, up)

                def forward_backward(fn):
                    return torch.autograd.grad(fn(*leaves, taps, up), leaves, g_out)

                if not records:
                    # the process's first seconds of backward calls run at half speed on the host for both implementations
                    # (observed: 0.19 - 0.27 ms a call against 0.10 from then on): spend them before the first window
                    t0 = time.perf_counter()
                    while time.perf_counter() - t0 < a.prewarm_s:
                        forward_backward(hip_tail), forward_backward(torch_tail)
                    torch.cuda.synchronize()
                for mode, run in (('forward', forward), ('forward+backward', forward_backward)):
                    (t_hip, t_ref), calls = alternate([lambda: run(hip_tail), lambda: run(torch_tail)], a.windows, a.window_ms)
                    got_hip, got_ref = run(hip_tail), run(torch_tail)
                    if mode == 'forward':
                        dist = float((got_hip - got_ref).abs().max())
                    else:
                        dist = max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(got_hip, got_ref))
                    hip, ref = spread(t_hip), spread(t_ref)
                    noise_band = max(hip['p90_ms'] - hip['p10_ms'], ref['p90_ms'] - ref['p10_ms'])
                    rec = dict(batch=batch, channels=c, resolution=r, up=up, mode=mode, windows=a.windows, calls_per_window=dict(hip=calls[0], pytorch=calls[1]), out_megabytes=4e-6 * batch * c * r * r,
                               hip=hip, pytorch=ref, ratio=ref['median_ms'] / hip['median_ms'], hip_vs_pytorch=dist,
                               slower=hip['median_ms'] > ref['median_ms'] + noise_band)
                    records.append(rec)
                    if rec['slower']:
                        slower.append((batch, c, r, up, mode))
                    print('synth tail [%d,%3d,%3d,%3d] %-5s %-16s: HIP %.4f ms (p10 %.4f, p90 %.4f), PyTorch %.4f ms (p10 %.4f, p90 %.4f), '
                          'ratio %.2f; HIP against PyTorch %.2e' % (batch, c, r, r, 'up' if up else 'plain', mode, hip['median_ms'], hip['p10_ms'],
                                                                     hip['p90_ms'], ref['median_ms'], ref['p10_ms'], ref['p90_ms'], rec['ratio'], dist),
                          flush=True)
                del y, g_out, leaves
                torch.cuda.empty_cache()
    print('HIP slower than PyTorch by more than the spread at: %s' % (slower or 'no shape and mode'))
    return dict(device=torch.cuda.get_device_name(0), shapes=SHAPES, batches=BATCHES, records=records, slower=slower)


def e2e_compare(a):
    import end_to_end as e2e
    dev = torch.device('cuda:0')
    out = {}
    for batch in a.batches:
        for leg in ('inversion', 'gstep'):
            runs = {'plain': [], 'fused_synthesis_tail': []}
            for _ in range(a.rounds):
                for name, fused in (('plain', False), ('fused_synthesis_tail', True)):
                    r = e2e.LEGS[leg](dev, 'hip', batch=batch, iters=a.iters, warmup=a.warmup, fused_synthesis_tail=fused)
                    runs[name].append({k: r[k] for k in ('ms_median', 'ms_min', 'ms_max')})
                    print('%s, %d image(s), %-20s: %.3f ms per step (min %.3f, max %.3f)' % (leg, batch, name, r['ms_median'], r['ms_min'],
                                                                                             r['ms_max']), flush=True)
                    torch.cuda.empty_cache()
            best = {k: min(x['ms_median'] for x in v) for k, v in runs.items()}
            out['%s_%d' % (leg, batch)] = dict(leg=leg, images=batch, runs=runs, iters=a.iters, best_median_ms=best,
                                               ratio=best['plain'] / best['fused_synthesis_tail'])
    return dict(device=torch.cuda.get_device_name(0), legs=out)


def one_leg(a):
    import end_to_end as e2e
    r = e2e.LEGS[a.leg](torch.device('cuda:0'), 'hip', iters=a.iters, warmup=a.warmup, markers=a.markers, fused_synthesis_tail=a.fused)
    r.update(leg=a.leg, impl='hip', texels='fp32', fused_synthesis_tail=a.fused)
    if a.sidecar:
        json.dump({'markers': e2e.MARKER_OPS, 'iters': a.iters, 'warmup': a.warmup, 'result': r}, open(a.sidecar, 'w'))
    print(json.dumps(r))
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=9, help='timed windows per implementation, shape and mode')
    ap.add_argument('--window-ms', type=float, default=30.0, help='length of a timed window: as many calls as fill it')
    ap.add_argument('--prewarm-s', type=float, default=3.0, help='seconds of untimed forward + backward calls before the first window')
    ap.add_argument('--warmup', type=int, default=3, help='legs: steps before the timed ones')
    ap.add_argument('--batches', type=int, nargs='+', default=[4, 1], help='--e2e: images per step')
    ap.add_argument('--e2e', action='store_true', help='the inversion and generator-step legs with and without attach(fused_synthesis_tail=True)')
    ap.add_argument('--leg', choices=('inversion', 'gstep'), help='one leg alone (for the profiler)')
    ap.add_argument('--fused', action='store_true', help='--leg: with attach(fused_synthesis_tail=True)')
    ap.add_argument('--markers', action='store_true')
    ap.add_argument('--sidecar')
    ap.add_argument('--iters', type=int, default=12)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_synth_tail: no GPU visible (there is no CPU path to time)')
    result = one_leg(a) if a.leg else e2e_compare(a) if a.e2e else micro(a)
    if a.out and result is not None:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(result, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
