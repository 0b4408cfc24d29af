"""CPU census of the render kernels' per-XCD hand-out: how many rays each of the 8 XCDs has to MARCH (rays that meet the
scene cube inflated by 1e-4, hit bit 1 of the ray set-up) when pixel block g = 8 * slot + q sits in queue q - today's order
(NFI_TUNING_XCD_BLOCKS_IN_ORDER) - and when the set-up's block table pairs heavy and light blocks (raygen_finish_kernel in
nfi_kernels.hip; paired_table below is the same rule).

  python tools/xcd_balance.py                       # the benchmark's own cameras: bench.synthetic_inputs(8, 1234)
  python tools/xcd_balance.py --seeds 0 1 2 --radius 2.0      # bench.cameras(8, radius, seed) per seed
  python tools/xcd_balance.py --seeds 0 --radius 1.3          # every ray hits

No GPU: rays and the slab test are the oracle's."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                  # noqa: E402
from oracle import nfi_oracle as orc          # noqa: E402

N_XCD = 8
INFLATE = 1.0001          # the inflated cube of the second slab test (raygen_kernel)


def block_side(height, width):
    """the block side of the per-XCD queues: the largest of 32 / 16 / 8 that divides both image sides (render_block_geometry)"""
    both = height | width
    return 32 if both % 32 == 0 else (16 if both % 16 == 0 else 8)


def marched_mask(cam, focal, height, width, scene_range):
    """bool [B, H, W]: the rays the kernel marches with skip_missed_rays"""
    ro, rd = orc.ray_bundle(height, width, focal, cam)
    _, _, hit = orc.near_far(ro, orc.unit_dirs(rd), scene_range * INFLATE)
    return hit


def block_counts(mask):
    """int64 [n_blocks]: marched rays per pixel block, blocks in image-major, row-major order (the kernel's block index)"""
    B, H, W = mask.shape
    s = block_side(H, W)
    assert H % s == 0 and W % s == 0, 'the per-XCD queues need image sides that are multiples of 8'
    return mask.view(B, H // s, s, W // s, s).sum(dim=(2, 4)).reshape(-1).to(torch.int64)


def paired_table(counts):
    """The block table: slot -> block.  Every COMPLETE aligned group G of 16 slots: its blocks ranked by (count descending,
    index ascending), rank r and rank 15 - r go to XCD (min(r, 15 - r) + G) % 8, the heavier first; identity elsewhere."""
    n = len(counts)
    table = list(range(n))
    for G in range(n // 16):
        order = sorted(range(16), key=lambda i: (-int(counts[16 * G + i]), i))
        for r, i in enumerate(order):
            x = (min(r, 15 - r) + G) % 8
            table[16 * G + (0 if r < 8 else 8) + x] = 16 * G + i
    return table


def per_xcd(counts, table=None):
    """marched rays per XCD: slot g belongs to XCD g % 8"""
    sums = [0] * N_XCD
    for g in range(len(counts)):
        sums[g % N_XCD] += int(counts[g if table is None else table[g]])
    return sums


def spread(sums):
    mean = sum(sums) / len(sums)
    return max(sums) / mean if mean > 0 else 1.0


def census(cam, focal, height, width, scene_range):
    counts = block_counts(marched_mask(cam, focal, height, width, scene_range))
    in_order, paired = per_xcd(counts), per_xcd(counts, paired_table(counts))
    bpi = len(counts) // cam.shape[0]
    scene = lambda table: [spread(per_xcd(counts[i * bpi:(i + 1) * bpi],
                                          None if table is None else [t - i * bpi for t in table[i * bpi:(i + 1) * bpi]]))
                           for i in range(cam.shape[0])] if bpi % 16 == 0 else []
    return dict(counts=counts, in_order=in_order, paired=paired, in_order_per_scene=scene(None),
                paired_per_scene=scene(paired_table(counts)))


def bench_cameras(seed, radius=None, n_images=bench.IMAGES_PER_GPU):
    """radius None: the cameras of bench.synthetic_inputs(n_images, seed) - the benchmark's own; else bench.cameras"""
    if radius is None:
        d = bench.synthetic_inputs(n_images, seed, 'cpu')
        return d['cam'], d['focal']
    return bench.cameras(n_images, radius, torch.Generator().manual_seed(seed)), torch.full((n_images,), bench.FOCAL)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--seeds', type=int, nargs='+', default=[1234])
    ap.add_argument('--radius', type=float, default=None, help='camera distance (default: the benchmark inputs of the seed)')
    ap.add_argument('--images', type=int, default=bench.IMAGES_PER_GPU)
    ap.add_argument('--size', type=int, default=bench.R)
    a = ap.parse_args(argv)
    worst = 0.0
    for seed in a.seeds:
        cam, focal = bench_cameras(seed, a.radius, a.images)
        c = census(cam, focal, a.size, a.size, bench.SCENE_RANGE)
        print('seed %d: %d of %d rays marched' % (seed, int(c['counts'].sum()), a.images * a.size * a.size))
        for name in ('in_order', 'paired'):
            ps = c[name + '_per_scene']
            print('  %-8s per XCD %s  max/mean %.3f%s' % (name, ' '.join('%d' % v for v in c[name]), spread(c[name]),
                  '  per scene: mean %.2f worst %.2f' % (sum(ps) / len(ps), max(ps)) if ps else ''))
        worst = max(worst, spread(c['paired']))
    print('paired order, worst max/mean over the seeds: %.3f' % worst)
    return 0


if __name__ == '__main__':
    sys.exit(main())
