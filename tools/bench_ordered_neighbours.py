"""Ordered against atomic backward of the two neighbours of the render node, HIP events on the launch stream, the two
entries alternating inside one process:   python tools/bench_ordered_neighbours.py [iterations]
  the augmentation warp at 60 x 6 x 128 x 128 (4 images x 15 copies of cat(prediction, target); the transforms are
  augment.draw_transform's at p = 0.8), and as the worst case of the gather every image zoomed out by 0.5;
  the fused hand-off backward at B = 4, 128 -> 96 channels, 256 x 256 (the last block of the 256^2 network)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from nerf_from_image_amd import _lib  # noqa: E402
if os.environ.get('NFI_PROBE_LIBRARY'):          # a variant build, as tools/bench_regulariser.py
    _lib.LIBRARY = os.environ['NFI_PROBE_LIBRARY']
from nerf_from_image_amd import augment, ops  # noqa: E402


def alternate(fns, n, warm=5):
    """Median ms of each of fns, called in turn n times (after `warm` rounds), and the last outputs."""
    for _ in range(warm):
        outs = [f() for f in fns]
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(n):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); outs[i] = f(); b.record()
            times[i].append((a, b))
    torch.cuda.synchronize()
    return [sorted(a.elapsed_time(b) for a, b in t)[n // 2] for t in times], outs


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    N, C, H, W = 60, 6, 128, 128
    g_out = torch.randn(N, C, H, W, device=dev)
    draws = augment.draw_transform(N, dev, 0.8, False)
    zoom_out = (draws[0], torch.full((N,), 0.5, device=dev), draws[2])
    for what, (rot, scale, shift) in (('draws at p = 0.8', draws), ('every image zoomed out by 0.5', zoom_out)):
        (t_atomic, t_ordered), (a, o) = alternate([lambda: ops.affine_warp_bwd(g_out, rot, scale, shift),
                                                   lambda: ops.affine_warp_bwd(g_out, rot, scale, shift, ordered=True)], n)
        again = ops.affine_warp_bwd(g_out, rot, scale, shift, ordered=True)
        print('warp backward %d x %d x %d x %d, %s: atomic %.3f ms, ordered %.3f ms, no workspace; repeat bit-identical: %s, against '
              'the atomic entry %.1e of its maximum' % (N, C, H, W, what, t_atomic, t_ordered, torch.equal(again, o),
                                                        float((a - o).abs().max() / a.abs().max())))

    B, Cin, R = 4, 128, 256
    x = torch.randn(B, Cin, R, R, device=dev)
    s = torch.randn(B, Cin, device=dev) / Cin ** 0.5
    w = torch.randn(96, Cin, device=dev)
    prev = torch.randn(B, 96, R // 2, R // 2, device=dev)
    g = torch.randn(B, 96, R, R, device=dev).contiguous(memory_format=torch.channels_last)
    (t_atomic, t_ordered), (a, o) = alternate([lambda: ops.torgb_texels_bwd(g, x, s, w, prev),
                                               lambda: ops.torgb_texels_bwd(g, x, s, w, prev, ordered=True)], n)
    again = ops.torgb_texels_bwd(g, x, s, w, prev, ordered=True)
    n_ws = _lib.struct_query('nfi_torgb_texels_bwd_ordered_workspace_bytes', 'nfi_torgb_args', n_scenes=B, in_channels=Cin, resolution=R)
    worst = max(float((a[k] - o[k]).abs().max() / a[k].abs().max()) for k in a)
    print('hand-off backward B = %d, %d -> 96 channels, %d x %d: atomic %.3f ms, ordered %.3f ms (both with their output allocations), '
          'workspace %.2f MiB; repeat bit-identical: %s, worst output against the atomic entry %.1e of its maximum' % (
              B, Cin, R, R, t_atomic, t_ordered, n_ws / 2 ** 20, all(torch.equal(again[k], o[k]) for k in o), worst))


if __name__ == '__main__':
    main()
