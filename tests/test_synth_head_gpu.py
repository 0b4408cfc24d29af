"""ops.synth_head / synth_head_bwd / synth_modulate / synth_modulate_bwd, synthesis.layer_styles / modulate /
fuse_layers(head=True) and attach(fused_synthesis_head=True) (csrc/nfi_synth_head.inc) on the GPU against the float64
restatement of tests/synth_head_util.py, which tests/test_synth_head_abi.py pins to the live reference classes.

The bound, per case and per quantity: max(2 x e32, 2^-21 x max(1, max |want|)).  e32 is the float32 restatement's own worst
distance to the float64 yardstick on the CPU (never the code under test); 2^-21 is the tail tests' floor, scaled by the
quantity's magnitude because styles and dcoefs are not O(1) (dcoefs reaches 1e4 where the styles vanish).

Head shapes (synth_head_util.HEAD_SHAPES): the five of the issue - (1,1,1,1,1); D = 70, one wave plus a tail; I K = 297, not
a multiple of 64; toRGB without demodulation and with style_gain = 1/8; the real largest layer (4,512,512,512,9) - and two
for the paths those do not take: 10 images (the kernels keep 8 images' sums per thread: two groups) with 19 rows (three
groups of 8 rows in the backward's pass over W), and K = 4 with I = 300 (the generic-K kernels; two blocks of 256 channels).

Modulate planes: 16, 25 (not a multiple of 4: the scalar path), 256, 4225 = 65^2 (scalar), one [1,2,256,256]; and the sides of
the backward's two switches of geometry - 16 lanes per plane up to 256 elements, a wave up to 2048, a block of 1024 above:
256 | 260 and 2048 | 2052."""
import pytest
import torch

from oracle import reference
import synth_head_util as hu

HEAD_NAMES = list(hu.HEAD_SHAPES)
MOD_BATCHES = [(1, 1), (2, 5), (3, 16)]
MOD_PLANES = [16, 25, 256, 260, 2048, 2052, 4225]


def on(dev, t):
    return None if t is None else t.to(dev)


def strided_rows(dev, latent):
    """latent as a layer sees it: row k of a [B,3,D] ws, a view with rows 3 D apart."""
    ws = torch.randn(latent.shape[0], 3, latent.shape[1], device=dev)
    ws[:, 1] = latent.to(dev)
    view = ws.unbind(1)[1]
    assert not view.is_contiguous() or latent.shape[0] == 1
    return view


class Affine:
    """What layer_styles reads of an EqualizedLinear."""

    def __init__(self, weight, bias, weight_gain, bias_gain):
        self.weight, self.bias, self.weight_gain, self.bias_gain = weight, bias, weight_gain, bias_gain


def run_head(dev, c, through, needs=hu.HEAD_GRADS):
    """One head case on the GPU: {quantity: tensor} - styles, dcoefs and the gradients in `needs` - through the C ABI
    wrappers or through the autograd node.  The latent is the strided view a layer passes."""
    from nerf_from_image_amd import ops, synthesis
    t, demod, sg = c['inputs'], c['demodulate'], c['style_gain']
    latent, A, a_bias, W = strided_rows(dev, t['latent']), on(dev, t['A']), on(dev, t['a_bias']), on(dev, t['W'])
    g_styles, g_dcoefs = on(dev, t['g_styles']), on(dev, t['g_dcoefs']) if demod else None
    needs = [n for n in needs if (n != 'g_weight' or demod) and (n != 'g_affine_bias' or a_bias is not None)]
    if through == 'abi':
        styles, dcoefs = ops.synth_head(latent, A, a_bias, t['weight_gain'], t['bias_gain'], W, demod, sg)
        got = ops.synth_head_bwd(g_styles, g_dcoefs, styles, dcoefs, latent, A, a_bias, t['weight_gain'], t['bias_gain'], W, demod, sg,
                                 need_latent='g_latent' in needs, need_affine_weight='g_affine_weight' in needs,
                                 need_affine_bias='g_affine_bias' in needs, need_weight='g_weight' in needs)
        assert set(got) == set(needs)
    else:
        # the latent is row 1 of a [B,3,D] leaf, as a layer gets it from ws.unbind(1): its gradient lands in that row alone
        ws = torch.randn(t['latent'].shape[0], 3, t['latent'].shape[1], device=dev)
        ws[:, 1] = t['latent'].to(dev)
        leaves = {'g_latent': ws, 'g_affine_weight': A.clone(), 'g_affine_bias': a_bias, 'g_weight': W.clone()}
        for n in needs:
            leaves[n] = leaves[n].clone().requires_grad_()
        styles, dcoefs = synthesis.layer_styles(leaves['g_latent'].unbind(1)[1], Affine(leaves['g_affine_weight'], leaves['g_affine_bias'],
                                                                                        t['weight_gain'], t['bias_gain']),
                                                leaves['g_weight'], demod, sg)
        target = (styles * g_styles).sum() + ((dcoefs * g_dcoefs).sum() if demod else 0.0)
        grads = torch.autograd.grad(target, [leaves[n] for n in needs])
        got = dict(zip(needs, grads))
        if 'g_weight' in got:
            got['g_weight'] = got['g_weight'].reshape(W.shape[0], W.shape[1], -1)
        if 'g_latent' in got:
            assert float(got['g_latent'][:, 0].abs().max()) == 0.0 and float(got['g_latent'][:, 2].abs().max()) == 0.0
            got['g_latent'] = got['g_latent'][:, 1].contiguous()
        styles, dcoefs = styles.detach(), None if dcoefs is None else dcoefs.detach()
    got['styles'] = styles
    if demod:
        got['dcoefs'] = dcoefs
    else:
        assert dcoefs is None
    return got


def check(got, c, label):
    """Asserts the bound for every quantity of `got`; returns the worst error / tolerance."""
    worst = 0.0
    for name, value in got.items():
        want = c['want'][name]
        assert value.dtype == torch.float32 and tuple(value.shape) == tuple(want.shape), (label, name, value.shape, want.shape)
        assert bool(torch.isfinite(value).all()), (label, name)
        err, tol = float((value.cpu().double() - want).abs().max()), hu.tolerance(c['e32'][name], want)
        assert err <= tol, (label, name, err, tol)
        worst = max(worst, err / tol)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize('name', HEAD_NAMES)
def test_head_parity_with_the_float64_restatement(gpu_device, name):
    B, D, I, O, K, demod, sg = hu.HEAD_SHAPES[name]
    c = hu.head_case(B, D, I, O, K, demod, sg)
    worst = 0.0
    for through in ('abi', 'node'):
        got = run_head(gpu_device, c, through)
        assert set(got) == set(c['want']), (through, set(got), set(c['want']))
        worst = max(worst, check(got, c, (name, through)))
    print('synth head parity %s (B, D, I, O, K) = %s: worst error / tolerance %.3f' % (name, (B, D, I, O, K), worst))


def run_modulate(dev, c, through, shape=None):
    from nerf_from_image_amd import ops, synthesis
    t = c['inputs']
    x, s, g_out = (on(dev, t[k]) for k in ('x', 'styles', 'g_out'))
    if shape is not None:
        x, g_out = x.reshape(shape), g_out.reshape(shape)
    if through == 'abi':
        out = ops.synth_modulate(x, s)
        g_x, g_s = ops.synth_modulate_bwd(g_out, x, s)
    else:
        x, s = x.clone().requires_grad_(), s.clone().requires_grad_()
        out = synthesis.modulate(x, s)
        g_x, g_s = torch.autograd.grad(out, (x, s), g_out)
        out = out.detach()
    assert out.shape == x.shape and g_x.shape == x.shape and out.is_contiguous()
    n = t['x'].shape
    return {'out': out.reshape(n), 'g_x': g_x.reshape(n), 'g_styles': g_s}


@pytest.mark.gpu
@pytest.mark.parametrize('B,C', MOD_BATCHES)
@pytest.mark.parametrize('n', MOD_PLANES)
def test_modulate_parity_with_the_float64_restatement(gpu_device, n, B, C):
    c = hu.modulate_case(B, C, n)
    side = int(round(n ** 0.5))
    shape = (B, C, side, side) if side * side == n else (B, C, 1, n)
    worst = max(check(run_modulate(gpu_device, c, through, shape), c, (B, C, n, through)) for through in ('abi', 'node'))
    print('synth modulate parity B=%d C=%d plane=%d: worst error / tolerance %.3f' % (B, C, n, worst))


@pytest.mark.gpu
def test_modulate_parity_at_the_largest_plane(gpu_device):
    c = hu.modulate_case(1, 2, 256 * 256)
    worst = max(check(run_modulate(gpu_device, c, through, (1, 2, 256, 256)), c, ('256x256', through)) for through in ('abi', 'node'))
    print('synth modulate parity [1,2,256,256]: worst error / tolerance %.3f' % worst)


@pytest.mark.gpu
def test_modulate_views_and_unaligned_planes(gpu_device):
    """A channels-last x is copied dense and gives the bits of the dense call; a dense x at an offset of 4 bytes into its
    buffer (not 16-byte aligned) is read in place on the scalar path."""
    from nerf_from_image_amd import ops
    c = hu.modulate_case(2, 5, 256)
    t = {k: on(gpu_device, v) for k, v in c['inputs'].items()}
    x, g = t['x'].reshape(2, 5, 16, 16), t['g_out'].reshape(2, 5, 16, 16)
    want = (ops.synth_modulate(x, t['styles']),) + ops.synth_modulate_bwd(g, x, t['styles'])
    cl = lambda v: v.contiguous(memory_format=torch.channels_last)
    shifted = lambda v: torch.cat([v.new_zeros(1), v.reshape(-1)])[1:].view(v.shape)
    for view in (cl, shifted):
        xv, gv = view(x), view(g)
        if view is shifted:
            assert xv.data_ptr() % 16 == 4 and xv.is_contiguous()
        got = (ops.synth_modulate(xv, t['styles']),) + ops.synth_modulate_bwd(gv, xv, t['styles'])
        assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
        # the scalar path adds a plane's products in another order than the 16-byte path: float64 sums, rounded once - one
        # unit in the last place at the most
        assert float((want[2] - got[2]).abs().max()) <= (0.0 if view is cl else 2.0 ** -23 * float(want[2].abs().max()))
    only_x = ops.synth_modulate_bwd(g, x, t['styles'], need_styles=False)
    only_s = ops.synth_modulate_bwd(g, x, t['styles'], need_x=False)
    assert only_x[1] is None and only_s[0] is None and torch.equal(only_x[0], want[1]) and torch.equal(only_s[1], want[2])


@pytest.mark.gpu
def test_zero_latent_and_bias_give_zero_styles_and_the_largest_dcoefs(gpu_device):
    """styles = 0 and dcoefs = rsqrt(1e-8) = 1e4; the output and every gradient finite and within the bound."""
    c = hu.head_case(3, 130, 33, 16, 9, True, 1.0, True, True)
    assert float(c['want']['styles'].abs().max()) == 0.0 and abs(float(c['want']['dcoefs'].min()) - 1e4) < 1e-6
    for through in ('abi', 'node'):
        got = run_head(gpu_device, c, through)
        assert float(got['styles'].abs().max()) == 0.0 and float((got['dcoefs'] - 1e4).abs().max()) <= hu.FLOOR * 1e4
        worst = check(got, c, ('zero', through))
    print('synth head, zero latent and bias: worst error / tolerance %.3f' % worst)


@pytest.mark.gpu
@pytest.mark.parametrize('demod', [True, False])
def test_a_null_affine_bias_works(gpu_device, demod):
    c = hu.head_case(2, 70, 5, 3, 9 if demod else 1, demod, 1.0 if demod else 0.25, False)
    assert 'g_affine_bias' not in c['want']
    for through in ('abi', 'node'):
        got = run_head(gpu_device, c, through)
        assert 'g_affine_bias' not in got
        check(got, c, ('no bias', demod, through))


@pytest.mark.gpu
def test_each_subset_of_gradients_gives_the_values_of_the_full_set(gpu_device):
    c = hu.head_case(*hu.HEAD_SHAPES['ten_images'])
    full = run_head(gpu_device, c, 'abi')
    for mask in range(1, 15):
        needs = [n for bit, n in enumerate(hu.HEAD_GRADS) if mask >> bit & 1]
        for through in ('abi', 'node'):
            got = run_head(gpu_device, c, through, needs)
            assert set(got) == set(needs) | {'styles', 'dcoefs'}
            for n in needs:
                assert torch.equal(got[n], full[n]), (needs, through, n)
    # one upstream gradient at a time: the two runs add up to the full gradient, each of the three rounded to float32 once
    from nerf_from_image_amd import ops
    t = c['inputs']
    dev_t = {k: on(gpu_device, v) for k, v in t.items() if torch.is_tensor(v)}
    args = (dev_t['latent'], dev_t['A'], dev_t['a_bias'], t['weight_gain'], t['bias_gain'], dev_t['W'])
    only_s = ops.synth_head_bwd(dev_t['g_styles'], None, full['styles'], full['dcoefs'], *args, need_weight=False)
    only_d = ops.synth_head_bwd(None, dev_t['g_dcoefs'], full['styles'], full['dcoefs'], *args)
    for n in ('g_latent', 'g_affine_weight', 'g_affine_bias'):
        both = only_s[n].double() + only_d[n].double()
        tol = 1.01 * 2.0 ** -24 * sum(float(v[n].abs().max()) for v in (only_s, only_d, full))
        assert float((both - full[n].double()).abs().max()) <= tol, n
    assert torch.equal(only_d['g_weight'], full['g_weight'])


@pytest.mark.gpu
def test_two_calls_give_the_same_bits(gpu_device):
    for name in ('odd_row', 'torgb', 'ten_images'):
        c = hu.head_case(*hu.HEAD_SHAPES[name])
        a, b, n = run_head(gpu_device, c, 'abi'), run_head(gpu_device, c, 'abi'), run_head(gpu_device, c, 'node')
        for k in a:
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], n[k]), (name, k)
    for plane in (25, 256, 2052, 4225):
        c = hu.modulate_case(3, 16, plane)
        a, b, n = (run_modulate(gpu_device, c, through) for through in ('abi', 'abi', 'node'))
        for k in a:
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], n[k]), (plane, k)


@pytest.mark.gpu
def test_the_nodes_are_first_order_only_and_absent_under_no_grad(gpu_device):
    from nerf_from_image_amd import synthesis
    c = hu.head_case(*hu.HEAD_SHAPES['wave_and_tail'])
    t = {k: on(gpu_device, v) for k, v in c['inputs'].items() if torch.is_tensor(v)}
    affine = Affine(t['A'], t['a_bias'], c['inputs']['weight_gain'], 1.0)
    w = t['latent'].clone().requires_grad_()
    styles, dcoefs = synthesis.layer_styles(w, affine, t['W'])
    assert styles.grad_fn is not None and dcoefs.grad_fn is not None
    with pytest.raises(RuntimeError, match='first-order only'):
        torch.autograd.grad(styles.sum() + dcoefs.sum(), w, create_graph=True)
    x = torch.randn(2, 5, 4, 4, device=gpu_device, requires_grad=True)
    out = synthesis.modulate(x, styles.detach())
    with pytest.raises(RuntimeError, match='first-order only'):
        torch.autograd.grad(out.sum(), x, create_graph=True)
    with torch.no_grad():
        styles, dcoefs = synthesis.layer_styles(w, affine, t['W'])
        assert styles.grad_fn is None and dcoefs.grad_fn is None and synthesis.modulate(x, styles).grad_fn is None
    styles, none = synthesis.layer_styles(t['latent'], affine, t['W'], demodulate=False)      # nothing requires a gradient: no node
    assert styles.grad_fn is None and none is None


@pytest.mark.gpu
def test_the_wrappers_refuse_wrong_dtypes_counts_and_devices_before_the_library(gpu_device, monkeypatch):
    from nerf_from_image_amd import _lib, ops
    c = hu.head_case(*hu.HEAD_SHAPES['wave_and_tail'])
    t = {k: on(gpu_device, v) for k, v in c['inputs'].items() if torch.is_tensor(v)}
    wg = c['inputs']['weight_gain']
    styles, dcoefs = ops.synth_head(t['latent'], t['A'], t['a_bias'], wg, 1.0, t['W'])
    x = torch.randn(2, 5, 4, 4, device=gpu_device)
    monkeypatch.setattr(_lib, 'call_struct', lambda *a, **k: pytest.fail('reached the library'))
    head = lambda **kw: ops.synth_head(*[kw.get(n, t[n]) for n in ('latent', 'A', 'a_bias')], wg, 1.0, kw.get('W', t['W']))
    bwd = lambda **kw: ops.synth_head_bwd(kw.get('g_styles', t['g_styles']), kw.get('g_dcoefs', t['g_dcoefs']), kw.get('styles', styles),
                                          kw.get('dcoefs', dcoefs), t['latent'], t['A'], t['a_bias'], wg, 1.0, t['W'], **kw.get('flags', {}))
    for name in ('latent', 'A', 'a_bias', 'W'):
        with pytest.raises(TypeError, match='float32'):
            head(**{name: t[name].double()})
        with pytest.raises(RuntimeError, match='GPU'):
            head(**{name: t[name].cpu()})
    for bad in (dict(A=t['A'][:, :-1]), dict(A=t['A'][:-1]), dict(a_bias=t['a_bias'][:-1]), dict(W=t['W'][:, :-1]), dict(latent=t['latent'][0])):
        with pytest.raises(ValueError):
            head(**bad)
    for bad in (dict(g_styles=t['g_styles'][:, :-1]), dict(g_dcoefs=t['g_dcoefs'][:1]), dict(styles=styles[:1]), dict(dcoefs=dcoefs[:, 1:]),
                dict(g_styles=None, g_dcoefs=None), dict(dcoefs=None), dict(g_dcoefs=None), dict(styles=None),
                dict(flags=dict(need_latent=False, need_affine_weight=False, need_affine_bias=False, need_weight=False))):
        with pytest.raises(ValueError):
            bwd(**bad)
    with pytest.raises(TypeError, match='float32'):
        bwd(g_styles=t['g_styles'].half())
    with pytest.raises(ValueError, match='finite'):
        ops.synth_head(t['latent'], t['A'], t['a_bias'], float('nan'), 1.0, t['W'])
    for call in (lambda: ops.synth_modulate(x, styles[:, :-1]), lambda: ops.synth_modulate(x[:, :, 0, 0].reshape(-1), styles),
                 lambda: ops.synth_modulate_bwd(x[:, :, :2], x, styles), lambda: ops.synth_modulate_bwd(x, x, styles, False, False)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError, match='float32'):
        ops.synth_modulate(x.double(), styles)
    with pytest.raises(RuntimeError, match='GPU'):
        ops.synth_modulate(x, styles.cpu())
    if torch.cuda.device_count() > 1:
        other = torch.device('cuda', (gpu_device.index or 0) ^ 1)
        with pytest.raises(ValueError, match='lives on'):
            head(A=t['A'].to(other))
        with pytest.raises(ValueError, match='lives on'):
            ops.synth_modulate(x, styles.to(other))


# ---------------------------------------------------------------------------------------------------------------------
# the real SynthesisNetwork
# ---------------------------------------------------------------------------------------------------------------------
def needs_reference():
    if not reference.available():
        pytest.skip('reference sources not staged: run oracle/make_ref.py (or __graft_entry__.build()) where the reference checkout exists')


@pytest.mark.gpu
@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('noise_mode', ['random', 'const'])
def test_network_fused_with_the_head_against_the_unfused_one(gpu_device, noise_mode, training):
    """The real SynthesisNetwork (w_dim 32, resolution 16, 96 image channels, channel_max 16) with fuse_layers(head=True)
    against the unfused network on the same noise, by tests/test_synth_tail_gpu.py's rule: a tensor T - the planes, the
    gradient of ws and of every parameter - is within max(2 x max|plain_T - T64|, 2^-21) of the float64 yardstick, tensors
    of fewer than FEW elements within no less than 2 x e32 x max|T64|, and e32 itself is float32 rounding (E32_NETWORK)."""
    from nerf_from_image_amd import handoff, synthesis
    needs_reference()
    stylegan = reference.modules().stylegan
    yardstick = hu.network_yardstick(stylegan, noise_mode, training)
    net, ws, weight = hu.small_network(stylegan)
    net, ws, weight = net.to(gpu_device), ws.to(gpu_device), weight.to(gpu_device)
    keys = list(net.state_dict().keys())
    originals = [m.forward for m in net.modules()]
    plain = hu.network_step(net, ws, weight, noise_mode, training)
    own = hu.network_distances(plain, yardstick)
    synthesis.fuse_layers(net, head=True)
    assert len(synthesis.fused_layers(net)) == 5 and len(synthesis.fused_output_layers(net)) == 3
    got = hu.network_distances(hu.network_step(net, ws, weight, noise_mode, training), yardstick)
    assert list(net.state_dict().keys()) == keys
    missed, worst, e32 = hu.network_rule(own, got)
    print('network fused with the head (%s, training=%s): %d tensors, worst fused error / tolerance %.3f (%s); unfused relative e32 %.3e'
          % (noise_mode, training, len(got), worst[0], worst[1], e32))
    assert not missed, missed
    assert e32 <= hu.E32_NETWORK, e32

    # a seeded run draws the same noise fused and unfused (the device generator this time): 2 + 1 of the unfused distance apart
    def seeded():
        torch.manual_seed(11)
        with torch.no_grad():
            return net(ws, noise_mode=noise_mode)
    a = seeded()
    with synthesis.unfused(net):
        b = seeded()
    planes_tol = max(3 * own['planes'][0], hu.FLOOR)
    assert float((a - b).abs().max()) <= planes_tol

    # with the hand-off's fused last block as well (its toRGB styles from the head node): still within the rule's bound
    handoff.fuse_last_block(net)
    both = hu.network_distances(hu.network_step(net, ws, weight, noise_mode, training), yardstick)
    missed, worst, _ = hu.network_rule(own, both)
    print('  with the fused last block: worst error / tolerance %.3f (%s)' % worst)
    assert not missed, missed
    handoff.unfuse_last_block(net)
    synthesis.unfuse_layers(net)
    assert [m.forward for m in net.modules()] == originals                       # unfuse_layers restores every forward
    assert synthesis.fused_layers(net) == [] and synthesis.fused_output_layers(net) == []
    restored = hu.network_step(net, ws, weight, noise_mode, training)
    assert float((restored[0] - plain[0]).abs().max()) <= hu.FLOOR and list(net.state_dict().keys()) == keys


def attached_models(gpu_device):
    from stand_in import StandInGenerator
    from nerf_from_image_amd import generator
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
    return generator.attach(model()), generator.attach(model(), fused_synthesis_head=True)


@pytest.mark.gpu
def test_attach_serves_path_length_from_the_original_forwards(gpu_device):
    """attach(fused_synthesis_head=True) implies the tail; a forward that asks for path_length - differentiated twice - runs
    every layer's and output layer's own forward and returns what a plain model returns, within 2 x E32_NETWORK of its largest
    value (tests/test_synth_tail_gpu.py's test of this name); a first-order node in that graph would raise.  Afterwards the
    fused forwards are back."""
    from nerf_from_image_amd import synthesis
    needs_reference()
    plain, fused = attached_models(gpu_device)
    z = torch.randn(2, 512, generator=torch.Generator().manual_seed(3)).to(gpu_device)
    assert synthesis.fused_layers(plain.synthesis_network) == [] and synthesis.fused_output_layers(plain.synthesis_network) == []
    layers, outs = synthesis.fused_layers(fused.synthesis_network), synthesis.fused_output_layers(fused.synthesis_network)
    assert len(layers) == 5 and len(outs) == 3 and synthesis.head_fused(fused.synthesis_network)
    results = []
    for m in (plain, fused):
        torch.manual_seed(5)
        ppl = m(None, z, ['path_length'])['path_length']
        assert ppl.shape == (2,) and ppl.requires_grad
        ppl.sum().backward()                                                        # the second differentiation
        results.append(ppl.detach())
    apart, scale = float((results[0] - results[1]).abs().max()), float(results[0].abs().max())
    print('path_length, model with the fused head against the plain one: %.3e apart, relative %.3e (bound %.3e)' % (apart, apart / scale, 2 * hu.E32_NETWORK))
    assert apart <= 2 * hu.E32_NETWORK * scale and float(results[0].abs().min()) > 0
    assert synthesis.fused_layers(fused.synthesis_network) == layers and synthesis.fused_output_layers(fused.synthesis_network) == outs
    assert all(m.forward.__func__ is synthesis.fused_layer_forward and m._nfi_fused_head for m in layers)
    assert all(m.forward.__func__ is synthesis.fused_output_forward for m in outs)


@pytest.mark.gpu
def test_attach_render_step_planes_and_ws_gradient(gpu_device):
    """The plane producer of a model attached with fused_synthesis_head=True against the plain attach, on the styles its own
    mapping network gives and frozen noise: the planes a render step samples and the gradient of sum(planes * weight) with
    respect to ws, by the network rule - each within max(2 x the plain model's own distance, 2^-21) of the same producer in
    float64 on the CPU."""
    needs_reference()
    import copy
    plain, fused = attached_models(gpu_device)
    z = torch.randn(2, 512, generator=torch.Generator().manual_seed(3)).to(gpu_device)
    weight = torch.randn(2, 96, 16, 16, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        ws0 = plain.mapping_network(z)[:, :plain.synthesis_network.num_ws].contiguous()
        assert torch.equal(ws0, fused.mapping_network(z)[:, :plain.synthesis_network.num_ws])

    def step(net, ws, weight):
        ws = ws.clone().requires_grad_()
        planes = net(ws, noise_mode='const')
        g_ws, = torch.autograd.grad((planes * weight).sum(), ws)
        return planes.detach().cpu().double(), g_ws.cpu().double()
    want = step(copy.deepcopy(plain.synthesis_network).cpu().double(), ws0.cpu().double(), weight.double())
    own, got = step(plain.synthesis_network, ws0, weight.to(gpu_device)), step(fused.synthesis_network, ws0, weight.to(gpu_device))
    for name, w64, a, b in zip(('planes', 'g_ws'), want, own, got):
        e_own, e_got = float((a - w64).abs().max()), float((b - w64).abs().max())
        tol = max(2 * e_own, hu.FLOOR)
        print('attach(fused_synthesis_head=True) %s: %.3e from float64, the plain attach %.3e (bound %.3e, scale %.3g)'
              % (name, e_got, e_own, tol, float(w64.abs().max())))
        assert e_got <= tol, (name, e_got, tol)
        assert e_own <= hu.E32_NETWORK * float(w64.abs().max()), (name, e_own)
