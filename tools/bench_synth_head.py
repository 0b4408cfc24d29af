"""The head of a synthesis layer as HIP nodes (synthesis.layer_styles + synthesis.modulate; csrc/nfi_synth_head.inc) against the
same expressions in PyTorch-ROCm on the same GPU, and the end-to-end legs of tools/end_to_end.py with
attach(fused_synthesis_tail=True) - the best there was - against attach(fused_synthesis_head=True), which adds the head:
    python tools/bench_synth_head.py [--windows 9] [--window-ms 30] [--batches 8 4 1] [--out times.json]
    python tools/bench_synth_head.py --e2e [--iters 12] [--rounds 2] [--batches 4 1] [--out e2e.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \\
        python tools/bench_synth_head.py --leg inversion [--head] --markers --sidecar side.json         (then tools/phase_split.py DIR side.json)

What is timed (default mode): everything SynthesisLayer.forward (models/stylegan.py:325-356) does before its convolution -
the affine (173-177), the demodulation coefficients (127-130) and x * styles (132) - at the shapes the real network has:
I = O = 512 at R = 8 .. 64, 256 at 128, 128 at 256, w_dim 512, 3x3 weights, and the toRGB head of the last block (128 -> 96,
1x1, no demodulation, styles times weight_gain; 372-380) at R = 256; at B = 8, 4 and 1; the latent is row 1 of a [B,3,512] ws,
as a layer gets it.  Forward alone (no gradient), and forward + backward to the latent and to x with the parameters frozen (an
inversion step) - the gradients of the parameters are a training step's and are timed as `forward+backward, training`.
The comparator restates those lines in torch - weight * gain, bias * gain, F.linear, the [B,O,I,3,3] product, square, sum,
rsqrt, x * styles - and imports nothing of the reference.

Method, as tools/bench_synth_tail.py: a timed window is one pair of device events around K back-to-back calls, K chosen per
shape and mode so that a window lasts about `--window-ms`; `--prewarm-s` seconds of untimed calls at the start, one warm-up
window each, then `--windows` timed windows in which the two implementations alternate within this one process; a figure is a
window's time / K, reported as the median, the 10th and the 90th percentile over the windows.  A shape counts as `slower` when
the nodes' median exceeds the PyTorch median by more than the wider of the two p10 .. p90 spreads.

--e2e: tools/end_to_end.py's inversion and generator-step legs on a model attached with fused_synthesis_tail=True and on one
attached with fused_synthesis_head=True, `--rounds` times each, alternating, at the legs' 4 images and at 1.  --leg: one such
leg alone, for the profiler, writing the sidecar tools/phase_split.py reads."""
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
from bench_synth_tail import alternate, spread  # noqa: E402

W_DIM = 512
# (name, in channels, out channels, taps per side, R, demodulate)
SHAPES = (('layer', 512, 512, 3, 8, True), ('layer', 512, 512, 3, 16, True), ('layer', 512, 512, 3, 32, True), ('layer', 512, 512, 3, 64, True),
          ('layer', 256, 256, 3, 128, True), ('layer', 128, 128, 3, 256, True), ('torgb', 128, 96, 1, 256, False))


class Affine:
    """An EqualizedLinear's state (stylegan.py:148-171): what both implementations read."""

    def __init__(self, weight, bias):
        self.weight, self.bias = weight, bias
        self.weight_gain, self.bias_gain = 1.0 / weight.shape[1] ** 0.5, 1.0


def torch_head(x, w, affine, conv_weight, demodulate, style_gain):
    """stylegan.py:173-177, 373, 127-130, 132 restated: (x * styles, dcoefs or None)."""
    styles = F.linear(w, affine.weight * affine.weight_gain, affine.bias * affine.bias_gain)
    if style_gain != 1.0:
        styles = styles * style_gain
    bs = x.shape[0]
    dcoefs = None
    if demodulate:
        wm = conv_weight.unsqueeze(0) * styles.reshape(bs, 1, -1, 1, 1)
        dcoefs = (wm.square().sum(dim=[2, 3, 4]) + 1e-8).rsqrt()
    return x * styles.reshape(bs, -1, 1, 1), dcoefs


def hip_head(x, w, affine, conv_weight, demodulate, style_gain):
    styles, dcoefs = synthesis.layer_styles(w, affine, conv_weight, demodulate, style_gain)
    return synthesis.modulate(x, styles), dcoefs


def micro(a):
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(0)
    records, slower = [], []
    for batch in a.batches:
        for name, cin, cout, k, r, demod in SHAPES:
            sg = 1.0 if demod else 1.0 / cin ** 0.5
            ws = torch.randn(batch, 3, W_DIM, device=dev, generator=g)
            x = torch.randn(batch, cin, r, r, device=dev, generator=g)
            affine_w, affine_b = torch.randn(cin, W_DIM, device=dev, generator=g), torch.ones(cin, device=dev)
            conv_w = torch.randn(cout, cin, k, k, device=dev, generator=g)
            g_out, g_d = torch.randn(batch, cin, r, r, device=dev, generator=g), torch.randn(batch, cout, device=dev, generator=g)

            def forward(fn):
                with torch.no_grad():
                    return fn(x, ws.unbind(1)[1], Affine(affine_w, affine_b), conv_w, demod, sg)

            def backward(fn, training):
                lw, lx = ws.clone().requires_grad_(), x.clone().requires_grad_()
                params = [t.clone().requires_grad_(training) for t in (affine_w, affine_b, conv_w)]
                out, dcoefs = fn(lx, lw.unbind(1)[1], Affine(params[0], params[1]), params[2], demod, sg)
                leaves = [lw, lx] + (params if demod else params[:2]) if training else [lw, lx]
                return torch.autograd.grad([out] + ([dcoefs] if demod else []), leaves, [g_out] + ([g_d] if demod else []))

            if not records:
                t0 = time.perf_counter()
                while time.perf_counter() - t0 < a.prewarm_s:
                    backward(hip_head, True), backward(torch_head, True)
                torch.cuda.synchronize()
            modes = (('forward', forward), ('forward+backward', lambda fn: backward(fn, False)),
                     ('forward+backward, training', lambda fn: backward(fn, True)))
            for mode, run in modes:
                (t_hip, t_ref), calls = alternate([lambda: run(hip_head), lambda: run(torch_head)], a.windows, a.window_ms)
                got_hip, got_ref = run(hip_head), run(torch_head)
                dist = max(float((p - q).abs().max() / q.abs().max().clamp_min(1e-30)) for p, q in zip(got_hip, got_ref) if p is not None)
                hip, ref = spread(t_hip), spread(t_ref)
                noise_band = max(hip['p90_ms'] - hip['p10_ms'], ref['p90_ms'] - ref['p10_ms'])
                rec = dict(batch=batch, kind=name, in_channels=cin, out_channels=cout, taps=k * k, resolution=r, mode=mode, windows=a.windows,
                           calls_per_window=dict(hip=calls[0], pytorch=calls[1]), hip=hip, pytorch=ref, ratio=ref['median_ms'] / hip['median_ms'],
                           hip_vs_pytorch_relative=dist, slower=hip['median_ms'] > ref['median_ms'] + noise_band)
                records.append(rec)
                if rec['slower']:
                    slower.append((batch, name, cin, r, mode))
                print('synth head B=%d %-5s %3d->%3d R=%3d %-26s: HIP %.4f ms (p10 %.4f, p90 %.4f), PyTorch %.4f ms (p10 %.4f, p90 %.4f), '
                      'ratio %.2f; HIP against PyTorch %.2e' % (batch, name, cin, cout, r, mode, hip['median_ms'], hip['p10_ms'], hip['p90_ms'],
                                                                 ref['median_ms'], ref['p10_ms'], ref['p90_ms'], rec['ratio'], dist), flush=True)
            del x, g_out, ws
            torch.cuda.empty_cache()
    print('HIP slower than PyTorch by more than the spread at: %s' % (slower or 'no shape and mode'))
    return dict(device=torch.cuda.get_device_name(0), shapes=SHAPES, batches=a.batches, records=records, slower=slower)


def e2e_compare(a):
    import end_to_end as e2e
    dev = torch.device('cuda:0')
    out = {}
    for batch in a.batches:
        for leg in ('inversion', 'gstep'):
            runs = {'fused_synthesis_tail': [], 'fused_synthesis_head': []}
            for _ in range(a.rounds):
                for name in runs:
                    r = e2e.LEGS[leg](dev, 'hip', batch=batch, iters=a.iters, warmup=a.warmup, **{name: True})
                    runs[name].append({k: r[k] for k in ('ms_median', 'ms_min', 'ms_max')})
                    print('%s, %d image(s), %-20s: %.3f ms per step (min %.3f, max %.3f)' % (leg, batch, name, r['ms_median'], r['ms_min'],
                                                                                             r['ms_max']), flush=True)
                    torch.cuda.empty_cache()
            best = {k: min(x['ms_median'] for x in v) for k, v in runs.items()}
            out['%s_%d' % (leg, batch)] = dict(leg=leg, images=batch, runs=runs, iters=a.iters, best_median_ms=best,
                                               ratio=best['fused_synthesis_tail'] / best['fused_synthesis_head'])
    return dict(device=torch.cuda.get_device_name(0), legs=out)


def one_leg(a):
    import end_to_end as e2e
    kw = {'fused_synthesis_head': True} if a.head else {'fused_synthesis_tail': True}
    r = e2e.LEGS[a.leg](torch.device('cuda:0'), 'hip', iters=a.iters, warmup=a.warmup, markers=a.markers, **kw)
    r.update(leg=a.leg, impl='hip', texels='fp32', **kw)
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
    ap.add_argument('--batches', type=int, nargs='+', default=None, help='images per call (default 8 4 1) or, with --e2e, per step (default 4 1)')
    ap.add_argument('--e2e', action='store_true', help='the inversion and generator-step legs with the fused tail alone and with the head as well')
    ap.add_argument('--leg', choices=('inversion', 'gstep'), help='one leg alone (for the profiler)')
    ap.add_argument('--head', action='store_true', help='--leg: with attach(fused_synthesis_head=True); without it, fused_synthesis_tail=True')
    ap.add_argument('--markers', action='store_true')
    ap.add_argument('--sidecar')
    ap.add_argument('--iters', type=int, default=12)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.batches is None:
        a.batches = [4, 1] if a.e2e else [8, 4, 1]
    if not torch.cuda.is_available():
        sys.exit('bench_synth_head: no GPU visible (there is no CPU path to time)')
    result = one_leg(a) if a.leg else e2e_compare(a) if a.e2e else micro(a)
    if a.out and result is not None:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(result, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
