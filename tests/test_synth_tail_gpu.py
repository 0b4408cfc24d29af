"""ops.synth_tail / ops.synth_tail_bwd / synthesis.layer_tail / synthesis.fuse_layers / attach(fused_synthesis_tail=True)
(csrc/nfi_synth_tail.inc) on the GPU against the float64 restatement of tests/synth_tail_util.py, which
tests/test_synth_tail_abi.py pins to the live SynthesisLayer.forward.

Sizes: layers without `up` at R = 4, 5 (R R not a multiple of 4: the scalar path) and 16; up layers at R = 2 (the smallest),
8 (inside a tile), 24 (not a power of two) and 64 (g_y, 65 x 65, spans 2 x 2 tiles); each at (B, C) = (1,1), (2,5), (3,16);
noise absent, [B,1,R,R] and [R,R]; activate on and off; the bilinear taps and an asymmetric, non-separable set.

The bound, per case and per quantity: max(2 x e32, 2^-21).  e32 is the float32 restatement's own worst distance to the
float64 yardstick on the CPU (never the code under test); 2^-21 is tests/test_blur_gpu.py's floor.  Gradients: the upstream
gradient is zero where |pre64| < 1e-3 std(pre64) - a float32 pre-activation that close to zero may sit on the other side of
the kink - so those elements drop out of g_y, g_noise and of both sides' sums for g_dcoefs and g_bias; their share stays under
0.5 % in every case (asserted; about 0.08 % for unit-normal inputs, test_synth_tail_abi.py)."""
import copy
import functools

import pytest
import torch

from oracle import reference
import synth_tail_util as su

SIZES = [(False, 4), (False, 5), (False, 16), (True, 2), (True, 8), (True, 24), (True, 64)]
BATCHES = [(1, 1), (2, 5), (3, 16)]
NOISES = (None, 'batch', 'shared')


def on(dev, t):
    return None if t is None else t.to(dev)


def run_case(dev, c, up, activate, through):
    """One case on the GPU: (out, {gradient name: tensor}), through the C ABI wrappers or through the autograd node."""
    from nerf_from_image_amd import ops, synthesis
    t = c['inputs']
    y, d, nz, b, taps = (on(dev, t[k]) for k in ('y', 'dcoefs', 'noise', 'bias', 'taps'))
    g_out = on(dev, c['g_out'])
    if through == 'abi':
        out = ops.synth_tail(y, d, nz, b, taps, c['gain'], up, activate)
        grads = ops.synth_tail_bwd(g_out, out, y, d, nz, b, taps, c['gain'], up, activate, need_noise=nz is not None)
        return out, grads
    leaves = [v.clone().requires_grad_() for v in (y, d, b) + ((nz,) if nz is not None else ())]
    out = synthesis.layer_tail(leaves[0], leaves[1], leaves[3] if nz is not None else None, leaves[2], taps, c['gain'], up, activate)
    got = torch.autograd.grad(out, leaves, g_out)
    return out.detach(), dict(zip(('g_y', 'g_dcoefs', 'g_bias', 'g_noise'), got))


def check_case(dev, key, up, activate, through):
    """Asserts the bound for the output and every gradient of one case; returns the worst error / tolerance ratio."""
    c = su.case(*key)
    assert c['excluded'] <= 0.005, (key, c['excluded'])
    out, grads = run_case(dev, c, up, activate, through)
    assert out.shape == c['out'].shape and out.dtype == torch.float32 and out.is_contiguous()
    worst = 0.0
    for name, got, want in [('out', out, c['out'])] + [(k, grads[k], c['grads'][k]) for k in c['grads']]:
        assert got.shape == want.shape, (key, name, got.shape, want.shape)
        err, tol = float((got.cpu().double() - want).abs().max()), su.tolerance(c['e32'][name])
        assert err <= tol, (key, through, name, err, tol)
        worst = max(worst, err / tol)
    assert set(grads) == set(c['grads'])
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize('B,C', BATCHES)
@pytest.mark.parametrize('up,R', SIZES)
def test_parity_with_the_float64_restatement(gpu_device, up, R, B, C):
    worst = 0.0
    for noise_kind in NOISES:
        for activate in (True, False):
            for taps_kind in (su.TAPS if up else ('bilinear',)):
                key = (B, C, R, up, noise_kind, activate, taps_kind)
                for through in ('abi', 'layer_tail'):
                    worst = max(worst, check_case(gpu_device, key, up, activate, through))
    print('synth tail parity up=%s R=%d B=%d C=%d: worst error / tolerance %.3f' % (up, R, B, C, worst))


@pytest.mark.gpu
@pytest.mark.parametrize('up,R', [(True, 8), (True, 64), (False, 5)])
def test_impulse_inputs(gpu_device, up, R):
    """y is a single 1.0 per plane at a corner, an edge and in the interior: the same bound, and the output is exactly the
    tail of zero farther than the taps reach."""
    worst = 0.0
    for place in su.IMPULSES:
        for taps_kind in (su.TAPS if up else ('bilinear',)):
            key = (2, 5, R, up, 'batch', True, taps_kind, 'impulse_' + place)
            worst = max(worst, check_case(gpu_device, key, up, True, 'abi'))
            if up:
                from nerf_from_image_amd import ops
                c = su.case(*key)
                t = c['inputs']
                zero = dict(t, y=torch.zeros_like(t['y']))
                args = lambda s: [on(gpu_device, s[k]) for k in ('y', 'dcoefs', 'noise', 'bias', 'taps')]
                got, flat = ops.synth_tail(*args(t), c['gain'], True).cpu(), ops.synth_tail(*args(zero), c['gain'], True).cpu()
                iy, ix = su.impulse_at(place, R + 1)
                i, j = torch.arange(R).view(R, 1), torch.arange(R).view(1, R)
                reach = (i >= iy - 2) & (i <= iy + 1) & (j >= ix - 2) & (j <= ix + 1)      # i + a - 1 = iy for a in 0..3
                assert torch.equal(got[..., ~reach], flat[..., ~reach]), (place, taps_kind)
                assert not torch.equal(got[..., reach], flat[..., reach])
    print('synth tail impulses up=%s R=%d: worst error / tolerance %.3f' % (up, R, worst))


@pytest.mark.gpu
@pytest.mark.parametrize('R', [180, 181, 184])
@pytest.mark.parametrize('noise_kind', ['batch', 'shared'])
def test_noise_gradient_on_both_sides_of_its_kernel_choice(gpu_device, R, noise_kind):
    """g_noise runs 16 pixels per block below 512 blocks of 64 pixels and 64 per block from there on: ceil(R R / 64) is
    507 at R = 180, 512 at R = 181 (R R odd: the last block is partial) and 529 at R = 184 (one image, or the shared form).
    Two channels keep the case small."""
    worst = check_case(gpu_device, (1, 2, R, False, noise_kind, True, 'bilinear'), False, True, 'abi')
    print('synth tail g_noise R=%d %s: worst error / tolerance %.3f' % (R, noise_kind, worst))


@pytest.mark.gpu
@pytest.mark.parametrize('up,R,noise_kind', [(True, 64, 'batch'), (True, 24, 'shared'), (False, 16, 'batch'), (False, 5, 'shared')])
def test_two_calls_give_the_same_bits(gpu_device, up, R, noise_kind):
    c = su.case(3, 16, R, up, noise_kind, True, 'asymmetric' if up else 'bilinear')
    out_a, grads_a = run_case(gpu_device, c, up, True, 'abi')
    out_b, grads_b = run_case(gpu_device, c, up, True, 'abi')
    out_c, grads_c = run_case(gpu_device, c, up, True, 'layer_tail')
    assert torch.equal(out_a, out_b) and torch.equal(out_a, out_c)
    for k in grads_a:
        assert torch.equal(grads_a[k], grads_b[k]) and torch.equal(grads_a[k], grads_c[k]), k


@pytest.mark.gpu
def test_the_node_is_first_order_only_and_skips_what_nobody_asks_for(gpu_device):
    from nerf_from_image_amd import synthesis
    c = su.case(2, 5, 8, True, 'batch', True)
    t = {k: on(gpu_device, v) for k, v in c['inputs'].items()}
    y = t['y'].clone().requires_grad_()
    out = synthesis.layer_tail(y, t['dcoefs'], t['noise'], t['bias'], t['taps'], c['gain'], True)
    with pytest.raises(RuntimeError, match='first-order only'):
        torch.autograd.grad(out.sum(), y, create_graph=True)
    out = synthesis.layer_tail(y, t['dcoefs'], t['noise'], t['bias'], t['taps'], c['gain'], True)
    g, = torch.autograd.grad(out, y, on(gpu_device, c['g_out']))                    # only g_y: no workspace, one launch
    assert float((g.cpu().double() - c['grads']['g_y']).abs().max()) <= su.tolerance(c['e32']['g_y'])
    with torch.no_grad():                                                            # no node without a gradient to ask for
        assert synthesis.layer_tail(t['y'], t['dcoefs'], t['noise'], t['bias'], t['taps'], c['gain'], True).grad_fn is None
    # a replaced filter buffer is honoured: other taps, another result
    other = synthesis.layer_tail(t['y'], t['dcoefs'], t['noise'], t['bias'], on(gpu_device, su.asymmetric_taps()), c['gain'], True)
    want = su.case(2, 5, 8, True, 'batch', True, 'asymmetric')
    assert float((other.cpu().double() - want['out']).abs().max()) <= su.tolerance(want['e32']['out'])


# ---------------------------------------------------------------------------------------------------------------------
# the real SynthesisNetwork
# ---------------------------------------------------------------------------------------------------------------------
def needs_reference():
    if not reference.available():
        pytest.skip('reference sources not staged: run oracle/make_ref.py (or __graft_entry__.build()) where the reference checkout exists')


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


# A tensor of the network test with fewer elements has no worst case of its own: the largest of n rounding errors is a
# sample maximum, and below a few dozen samples two draws of it differ by more than the rule's factor of 2 too often.
FEW = 32
# float32 rounding through the network, relative to a tensor's largest magnitude: 2^-24 per operation, sums of up to
# 16 x 9 = 144 products (12 x as a random walk), 4 standard deviations for the worst of some 10^4 elements, 12 stages forward
# and backward (3.5 x as a random walk): about 170 x 2^-24, rounded up to 2^-16
E32_NETWORK = 2.0 ** -16


def small_network(seed=0):
    stylegan = reference.modules().stylegan
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


@functools.lru_cache(maxsize=None)
def network_yardstick(noise_mode, training):
    net, ws, weight = small_network()
    return network_step(copy.deepcopy(net).double(), ws.double(), weight.double(), noise_mode, training)


@pytest.mark.gpu
@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('noise_mode', ['random', 'const'])
def test_fused_network_against_the_unfused_one(gpu_device, noise_mode, training):
    """The real SynthesisNetwork (w_dim 32, resolution 16, 96 image channels, channel_max 16), fused against unfused on the
    same noise.  The bound for a tensor T - the planes, the gradient of ws and of every parameter - is the rule of the kernel
    tests with the UNFUSED network's own float32-against-float64 distance in e32's place: max(2 x max|plain_T - T64|, 2^-21).
    A tensor of fewer than FEW elements (a layer's bias gradient, the one-element noise_strength gradient) has no worst
    case of its own to speak of; its bound is no smaller than 2 x e32 x max|T64|, e32 being the unfused network's worst
    distance relative to the tensor's largest magnitude over the tensors that do - and that figure is asserted to be
    float32 rounding (E32_NETWORK)."""
    from nerf_from_image_amd import handoff, synthesis
    needs_reference()
    planes64, grads64 = network_yardstick(noise_mode, training)
    net, ws, weight = small_network()
    net, ws, weight = net.to(gpu_device), ws.to(gpu_device), weight.to(gpu_device)
    keys = list(net.state_dict().keys())
    plain = network_step(net, ws, weight, noise_mode, training)
    synthesis.fuse_layers(net)
    fused = network_step(net, ws, weight, noise_mode, training)
    assert list(net.state_dict().keys()) == keys

    def distances(run):
        """{name: (worst distance to the float64 yardstick, the yardstick's largest magnitude, elements)}"""
        out = {'planes': (float((run[0].cpu().double() - planes64).abs().max()), float(planes64.abs().max()), planes64.numel())}
        for k, g64 in grads64.items():
            assert (g64 is None) == (run[1][k] is None), k
            if g64 is not None:
                out[k] = (float((run[1][k].cpu().double() - g64).abs().max()), float(g64.abs().max()), g64.numel())
        return out
    own, got = distances(plain), distances(fused)
    # the fall-back for the tensors too small to have a worst case: the unfused network's worst distance relative to the
    # tensor's largest magnitude, over the tensors that are large enough
    e32 = max(err / scale for err, scale, n in own.values() if scale > 0 and n >= FEW)
    worst, missed = (0.0, None), []
    for k, (err, scale, n) in got.items():
        tol = max(2 * own[k][0], su.FLOOR)
        if n < FEW:
            tol = max(tol, 2 * e32 * scale)
        if err > tol:
            missed.append((k, n, err, tol))
        worst = max(worst, (err / tol, k))
    print('fused network (%s, training=%s): %d tensors, worst fused error / tolerance %.3f (%s); unfused relative e32 of the tensors '
          'with %d elements or more %.3e' % (noise_mode, training, len(got), worst[0], worst[1], FEW, e32))
    assert not missed, missed
    assert e32 <= E32_NETWORK, e32

    # a seeded run draws the same noise fused and unfused: the device generator this time
    def seeded():
        torch.manual_seed(11)
        with torch.no_grad():
            return net(ws, noise_mode=noise_mode)
    a = seeded()
    with synthesis.unfused(net):
        b = seeded()
    # no yardstick for this noise: fused within its bound of the truth and unfused within its own distance, so 2 + 1 apart
    planes_tol = max(3 * own['planes'][0], su.FLOOR)
    assert float((a - b).abs().max()) <= planes_tol

    # with the hand-off's fused last block on top: against the same block over unfused layers
    handoff.fuse_last_block(net)
    both = seeded()
    with synthesis.unfused(net):
        last_only = seeded()
    assert both.shape == last_only.shape == (2, 96, 16, 16)
    assert float((both - last_only).abs().max()) <= planes_tol
    both_grad = network_step(net, ws, weight, noise_mode, training)[1]
    assert all(torch.isfinite(g).all() for g in both_grad.values() if g is not None)


@pytest.mark.gpu
def test_attach_serves_path_length_from_the_unfused_layers(gpu_device):
    """attach(fused_synthesis_tail=True): a forward that asks for path_length - differentiated twice - runs the layers' own
    forwards and returns what an unfused model returns: the same ops on the same seed, each run within float32 rounding
    through the network (E32_NETWORK, relative to the largest value) of the exact result, so the two are at most twice that
    apart (the observed difference is printed); a first-order node inside that graph would raise instead.  After the call the
    layers are fused again."""
    from stand_in import StandInGenerator
    from nerf_from_image_amd import generator, synthesis
    needs_reference()
    stylegan = reference.modules().stylegan

    def model():
        torch.manual_seed(0)
        m = StandInGenerator(0.55, attention_values=0, use_sdf=True, plane_res=16)
        m.synthesis_network = stylegan.SynthesisNetwork(w_dim=512, img_resolution=16, img_channels=96, channel_max=16)
        with torch.no_grad():
            for name, p in m.synthesis_network.named_parameters():
                if name.endswith('noise_strength'):
                    p.fill_(0.3)
        return m.to(gpu_device).train()
    z = torch.randn(2, 512, generator=torch.Generator().manual_seed(3)).to(gpu_device)
    plain, fused = generator.attach(model()), generator.attach(model(), fused_synthesis_tail=True)
    assert synthesis.fused_layers(plain.synthesis_network) == []
    layers = synthesis.fused_layers(fused.synthesis_network)
    assert len(layers) == 5
    results = []
    for m in (plain, fused):
        torch.manual_seed(5)
        out = m(None, z, ['path_length'])
        ppl = out['path_length']
        assert ppl.shape == (2,) and ppl.requires_grad
        ppl.sum().backward()                                                        # the second differentiation
        results.append(ppl.detach())
    apart, scale = float((results[0] - results[1]).abs().max()), float(results[0].abs().max())
    print('path_length fused against unfused model: %.3e apart, relative %.3e (bound %.3e)' % (apart, apart / scale, 2 * E32_NETWORK))
    assert apart <= 2 * E32_NETWORK * scale
    assert float(results[0].abs().min()) > 0
    assert synthesis.fused_layers(fused.synthesis_network) == layers
    assert all(m.forward.__func__ is synthesis.fused_layer_forward for m in layers)
    # and a first-order forward of the fused model runs the HIP node
    torch.manual_seed(5)
    planes = fused.synthesis_network(fused.mapping_network(z)[:, :14], noise_mode='const')
    assert planes.grad_fn is not None and planes.shape == (2, 96, 16, 16)
    planes.sum().backward()
