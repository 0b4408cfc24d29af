"""Bit identity of two builds of the field backward (a refactor must not move a bit): sha256 of the output tensors.

    python tools/probes/bwd_bit_identity.py hash <libnfi_hip.so> <out.json>     # on the GPU, once per library
    python tools/probes/bwd_bit_identity.py compare <a.json> <b.json>

(1) g_points of the eight COORD kernels at the shape of test_backward_outputs_without_atomics_are_bit_reproducible, both
scatter modes, points_only, points_only + normalize_points; (2) every output of all 16 kernels at B = 1, P = 64 (one
working wave: its atomics are ordered) with per-point mixed scales, both scatter modes.  g_texels of the binned scatter is
NOT reproducible from launch to launch (bin_reduce adds a cell's partial sums from several half-waves with atomics): it is
launched eight more times, the number of distinct hashes is recorded, and it is compared with the atomic scatter by value.
Record of round 10: profiles/r10/bit_identity_{parent,new}.json.

    python tools/probes/bwd_bit_identity.py hash-ordered <libnfi_hip.so> <out.json>

The ordered (bit-reproducible) backwards, whose every output is a pure function of its inputs: ops.torgb_texels_bwd(ordered=True)
at the SHAPES of tests/test_handoff_warp_ordered.py with and without a previous image (and g_x / g_previous_image of the
atomic entry: one writer per element), ops.sdf_gradient_bwd(ordered=True) at the launches of tests/test_regulariser_ordered.py
and scatter_mode 2 at the cases of test_ordered_mode_repeats_bit_for_bit; inputs as those tests draw them.  `compare` as above.
Record of round 20: profiles/r20/ordered_bits_{parent,tree}.json."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def hash_outputs(lib, out_path):
    import torch
    from nerf_from_image_amd import _lib
    _lib.LIBRARY = os.path.abspath(lib)
    from nerf_from_image_amd import ops
    from nerf_from_image_amd.field_backward import field_query_bwd
    dev = torch.device('cuda:0')
    TEX = {0: ops.TEXEL_F32, 1: ops.TEXEL_BF16, 2: ops.TEXEL_F16}

    def sha(t):
        return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]

    def scene(seed, B, P, res, A, vd, tex, spr, mixed):
        g = torch.Generator().manual_seed(seed)
        n_out = 33 if vd else (1 + A if A > 0 else 4)
        planes = torch.randn(B, 3, 32, res, res, generator=g).to(dev)
        w1, b1 = torch.randn(64, 32, generator=g).to(dev), (0.3 * torch.randn(64, generator=g)).to(dev)
        w2, b2 = torch.randn(n_out, 64, generator=g).to(dev), (0.3 * torch.randn(n_out, generator=g)).to(dev)
        x = ((torch.rand(B, P, 3, generator=g) * 2 - 1) * 0.55 * 1.15).to(dev)
        att = (torch.rand(B, A, 3, generator=g) * 2 - 1).to(dev) if A > 0 else None
        beta, alpha = torch.tensor([0.12], device=dev), torch.tensor([0.3], device=dev)
        gs, gr = torch.randn(B, P, generator=g), torch.randn(B, P, 3, generator=g)
        if mixed:
            ps = 10.0 ** (torch.rand(B, P, generator=g) * 13 - 9)
            gs, gr = gs * ps, gr * ps[..., None]
        gs, gr = gs.to(dev), gr.to(dev)
        texels = ops.planes_to_texels(planes, TEX[tex])
        vda = None
        if vd:
            n3 = A if A > 0 else 3
            w3, b3 = torch.randn(n3, 32, generator=g).to(dev), (0.3 * torch.randn(n3, generator=g)).to(dev)
            xr = torch.randn(B, P // spr, 32, generator=g).to(dev)
            image = ops.decoder_pack_viewdir(w1, b1, w2, b2, w3, b3, A, TEX[tex])
            vda = dict(ray_features=ops.pad_ray_features(xr), samples_per_ray=spr, w3=w3)
        else:
            image = ops.decoder_pack(w1, b1, w2, b2, A, TEX[tex])

        def run(**kw):
            return field_query_bwd(x, texels, image, w1, w2, 0.55, A, att, True, beta, alpha, gs, gr, viewdir=vda, **kw)
        return run

    out = {}
    KERNELS = [(att, vd, tex) for att in (0, 1) for vd, tex in ((0, 0), (0, 1), (0, 2), (1, 0))]
    # (1) g_points of the eight COORD kernels, the shape of test_backward_outputs_without_atomics_are_bit_reproducible
    for att, vd, tex in KERNELS:
        run = scene(70500 + 10 * att + tex + 5 * vd, 2, 70000, 64, 10 if att else 0, vd, tex, 7, False)
        key = 'g_points <%d,1,%d,%d>' % (att, vd, tex)
        out[key + ' scatter 0'] = sha(run(want_points=True, scatter_mode=0)['g_points'])
        out[key + ' scatter 1'] = sha(run(want_points=True, scatter_mode=1)['g_points'])
        out[key + ' points_only'] = sha(run(points_only=True)['g_points'])
        out[key + ' points_only normalized'] = sha(run(points_only=True, normalize_points=True)['g_points'])
    # (2) every output at B = 1, P = 64 (one working wave: the atomics are ordered), per-point mixed scales, all 16 kernels
    for att, vd, tex in KERNELS:
        for coord in (0, 1):
            run = scene(64000 + 10 * att + tex + 5 * vd, 1, 64, 24, 10 if att else 0, vd, tex, 8, True)
            for mode in (0, 1):
                got = run(want_points=bool(coord), scatter_mode=mode)
                for k in sorted(got):
                    out['<%d,%d,%d,%d> scatter %d %s' % (att, coord, vd, tex, mode, k)] = sha(got[k])
                if mode == 1:
                    # the binned reduce sums a cell from several half-waves with atomics: is its g_texels reproducible at all?
                    reps = sorted(set(sha(run(want_points=bool(coord), scatter_mode=1)['g_texels']) for _ in range(8)))
                    out['<%d,%d,%d,%d> scatter 1 g_texels, distinct hashes in 8 more launches' % (att, coord, vd, tex)] = len(reps)
                    ref0 = run(want_points=bool(coord), scatter_mode=0)['g_texels'].double()
                    d = float((got['g_texels'].double() - ref0).abs().max() / ref0.abs().max())
                    out['<%d,%d,%d,%d> scatter 1 g_texels within 2e-5 of scatter 0' % (att, coord, vd, tex)] = bool(d <= 2e-5)
    torch.cuda.synchronize()
    json.dump(out, open(out_path, 'w'), indent=1, sort_keys=True)
    print('%s: %d hashes' % (lib, len(out)))


def hash_ordered(lib, out_path):
    import torch
    from nerf_from_image_amd import _lib
    _lib.LIBRARY = os.path.abspath(lib)
    from nerf_from_image_amd import ops
    from nerf_from_image_amd.field_backward import field_query_bwd
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_handoff_warp_ordered as tho
    import test_ordered_backward as tob
    import test_regulariser_operator as tro
    import test_regulariser_ordered as trd
    dev = torch.device('cuda:0')

    def sha(t):
        return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]

    out = {}
    for shape in tho.SHAPES:
        B, Cin, R = shape
        g = torch.Generator().manual_seed(B * 1000 + Cin + R)            # handoff_case's draws, without its float64 reference
        t = dict(x=torch.randn(B, Cin, R, R, generator=g), s=torch.randn(B, Cin, generator=g) / Cin ** 0.5,
                 w=torch.randn(96, Cin, generator=g), bias=torch.randn(96, generator=g),
                 prev=torch.randn(B, 96, R // 2, R // 2, generator=g), up=torch.randn(B, 96, R, R, generator=g))
        for has_prev in (False, True):
            for k, v in sorted(tho.handoff_bwd(t, dev, has_prev, True, True).items()):
                out['torgb ordered %s prev %d %s' % (shape, has_prev, k)] = sha(v)
            atomic = tho.handoff_bwd(t, dev, has_prev, True, False)
            for k in ('g_x', 'g_previous_image'):
                if k in atomic:
                    out['torgb atomic %s prev %d %s' % (shape, has_prev, k)] = sha(atomic[k])
    for name, interleaved in trd.LAUNCHES:
        c = tro.CASE[name]
        t = tro.scene(c)
        texels = tro.texels_of(t, dev, interleaved)
        got = ops.sdf_gradient_bwd(t['x'].to(dev), texels, t['w1'].to(dev), t['b1'].to(dev), t['w2'].to(dev), t['b2'].to(dev),
                                   tro.range_of(c), t['u_d'].to(dev), t['u_g'].to(dev), ordered=True)
        for k, v in sorted(got.items()):
            out['sdf_gradient ordered %s%s %s' % (name, ' interleaved' if interleaved else '', k)] = sha(v)
    cases = [m for m in tob.test_ordered_mode_repeats_bit_for_bit.pytestmark if m.name == 'parametrize'][0].args[1]
    for i, (B, P, kw, ray_order) in enumerate(cases):
        got = field_query_bwd(*tob.scatter_case(dev, P, 24, B=B, **kw), want_points=True, scatter_mode=2, ray_order=ray_order)
        for k, v in sorted(got.items()):
            out['field scatter 2 case %d %s' % (i, k)] = sha(v)
    torch.cuda.synchronize()
    json.dump(out, open(out_path, 'w'), indent=1, sort_keys=True)
    print('%s: %d hashes' % (lib, len(out)))


def compare(pa, pb):
    a, b = json.load(open(pa)), json.load(open(pb))
    skip = lambda k: 'distinct hashes' in k or (k.endswith('scatter 1 g_texels') and (a.get(k + ', distinct hashes in 8 more launches', 1) > 1))
    print('scatter 1 g_texels not reproducible launch to launch within ONE library: parent %d of 16 set-ups, new %d of 16' % (
        sum(v > 1 for k, v in a.items() if 'distinct hashes' in k), sum(v > 1 for k, v in b.items() if 'distinct hashes' in k)))
    print('scatter 1 g_texels within 2e-5 of scatter 0: parent %s, new %s' % (all(v for k, v in a.items() if 'within 2e-5' in k), all(v for k, v in b.items() if 'within 2e-5' in k)))
    print('skipped (unordered atomics of the binned reduce, parent varies by itself):', sum(skip(k) for k in a))
    bad = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k) and not skip(k)]
    print('bit identity: %d hashes compared, %d differ' % (len(a), len(bad)))
    for k in bad:
        print('  DIFFERS', k, a.get(k), b.get(k))
    sys.exit(1 if bad or len(a) != len(b) else 0)


if __name__ == '__main__':
    if sys.argv[1] == 'hash':
        hash_outputs(sys.argv[2], sys.argv[3])
    elif sys.argv[1] == 'hash-ordered':
        hash_ordered(sys.argv[2], sys.argv[3])
    else:
        compare(sys.argv[2], sys.argv[3])
