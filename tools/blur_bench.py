"""filters.blur against the reference's own ops.blur (lib/ops.py:42-55) under PyTorch-ROCm on the same GPU:
    python tools/blur_bench.py [--calls 200] [--warmup 20] [--out times.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/blur_bench.py --trace hip        (or: reference)

Shapes [4,4,128,128] (one replica's discriminator batch), [32,4,128,128] and [8,4,256,256], each fed as run.py:1090 feeds it:
a dense [B,H,W,C] batch behind permute(0,3,1,2), white background.  Iterations 0, 6250 and 12000 (r = 30, 15, 1).
Method: device events around each call on the launch stream, `--warmup` rounds first, then `--calls` timed rounds in which
the two implementations alternate within this one process; per figure the median, the 10th and 90th percentile.  Also the
largest distance of either output to the float64 restatement (two 1-D passes, on the CPU).

--trace hip | reference: a run of its own for the profiler, no timing: the named implementation alone makes 10 calls per
shape and iteration and nothing else touches the device, so the kernel trace's call counts divide by 10 x 9 = 90 into
launches per call (python tools/kstats.py DIR prints them)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from nerf_from_image_amd import filters  # noqa: E402
from oracle import reference  # noqa: E402

SHAPES = ((4, 4, 128, 128), (32, 4, 128, 128), (8, 4, 256, 256))
ITERATIONS = (0, 6250, 12000)
WARMUP_ITERS = 12500
TRACE_CALLS = 10


def float64_blur(x, i, white):
    sigma, r = filters.blur_schedule(i, WARMUP_ITERS)
    x = x.cpu()
    k = torch.arange(-r, r + 1, dtype=torch.float64)
    f = torch.exp2(-(k / sigma) ** 2)
    f = f / f.sum()
    b, c, h, w = x.shape
    bg = 1.0 if white else 0.0
    planes = (x.double() - bg).reshape(b * c, 1, h, w)
    rows = F.conv2d(planes, f.view(1, 1, 1, -1), padding=(0, r))
    return F.conv2d(rows, f.view(1, 1, -1, 1), padding=(r, 0)).view(b, c, h, w) + bg


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
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--trace', choices=('hip', 'reference'), default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    ref_blur = reference.modules().ops.blur
    g = torch.Generator().manual_seed(0)
    white = True
    records, slower = [], []
    for B, C, H, W in SHAPES:
        x = torch.rand(B, H, W, C, generator=g).to(dev).permute(0, 3, 1, 2)
        for i in ITERATIONS:
            sigma, r = filters.blur_schedule(i, WARMUP_ITERS)
            hip = lambda: filters.blur(x, i, WARMUP_ITERS, white)
            ref = lambda: ref_blur(x, i, WARMUP_ITERS, white)
            if a.trace:
                for _ in range(TRACE_CALLS):
                    (hip if a.trace == 'hip' else ref)()
                torch.cuda.synchronize()
                print('trace: %d calls of %s at %s, i = %d' % (TRACE_CALLS, a.trace, (B, C, H, W), i), flush=True)
                continue
            t_hip, t_ref = alternate([hip, ref], a.calls, a.warmup)
            want = float64_blur(x, i, white)
            rec = dict(shape=[B, C, H, W], i=i, radius=r, calls=a.calls, hip=spread(t_hip), reference=spread(t_ref),
                       ratio=t_ref[len(t_ref) // 2] / t_hip[len(t_hip) // 2],
                       hip_error=float((hip().cpu().double() - want).abs().max()),
                       reference_error=float((ref().cpu().double() - want).abs().max()))
            records.append(rec)
            if rec['ratio'] < 1.0:
                slower.append((rec['shape'], i))
            print('blur %s i = %5d (r = %2d): HIP %.4f ms (p10 %.4f, p90 %.4f), reference %.4f ms (p10 %.4f, p90 %.4f), ratio %.2f; '
                  'distance to float64: HIP %.2e, reference %.2e' % (
                      (B, C, H, W), i, r, rec['hip']['median_ms'], rec['hip']['p10_ms'], rec['hip']['p90_ms'], rec['reference']['median_ms'],
                      rec['reference']['p10_ms'], rec['reference']['p90_ms'], rec['ratio'], rec['hip_error'], rec['reference_error']), flush=True)
    if a.trace:
        return
    print('HIP slower than the reference at: %s' % (slower or 'no shape and iteration'))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(dict(device=torch.cuda.get_device_name(0), records=records, slower=slower), open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
