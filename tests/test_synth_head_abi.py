"""CPU-side checks of the synthesis-layer head (csrc/nfi_synth_head.inc, nerf_from_image_amd/synthesis.py): the entries are
exported with the header's prototypes and refuse what the header says they refuse - with the argument named, before any
launch; the workspace query returns 0 for a refused shape; the ops wrappers and the nodes refuse host tensors before the
library (a wrong dtype, count or second device needs device tensors: tests/test_synth_head_gpu.py); attach has the option, off; fuse_layers(head=True) / unfuse_layers / unfused swap and restore the forward
of every layer and output layer of the LIVE reference SynthesisNetwork; and the tests' own yardstick
(tests/synth_head_util.py) is the live EqualizedLinear / SynthesisLayer.forward / OutputLayer.forward, and the factored
demodulation the kernels evaluate equals stylegan.py:127-130 in float64."""
import ctypes
import functools
import inspect
import re

import pytest
import torch
import torch.nn.functional as F

from nerf_from_image_amd import _lib
from oracle import reference
import synth_head_util as hu
import synth_tail_util as su

needs_reference = pytest.mark.skipif(not reference.available(), reason='reference sources not available (oracle/make_ref.py)')
HEAD, MOD = 'nfi_synth_head_args', 'nfi_synth_modulate_args'
H_FWD, H_BWD, H_SIZE = 'nfi_synth_head_fwd', 'nfi_synth_head_bwd', 'nfi_synth_head_bwd_workspace_bytes'
M_FWD, M_BWD = 'nfi_synth_modulate_fwd', 'nfi_synth_modulate_bwd'


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    return _lib.load()


def test_entries_are_exported_with_the_header_prototypes(lib):
    src = _lib._strip_comments(open(_lib.HEADER).read())
    found = {m.group(2): (m.group(1), [p.strip() for p in m.group(3).split(',')])
             for m in re.finditer(r'(\w+)\s+(nfi_synth_(?:head|modulate)\w*)\s*\(([^)]*)\)\s*;', src)}
    head, mod = ['const %s* a' % HEAD, 'nfi_stream_t stream'], ['const %s* a' % MOD, 'nfi_stream_t stream']
    assert found == {H_FWD: ('int', head), H_BWD: ('int', head), H_SIZE: ('size_t', ['const %s* a' % HEAD]), M_FWD: ('int', mod),
                     M_BWD: ('int', mod)}
    for name in (H_FWD, H_BWD, M_FWD, M_BWD):
        assert _lib.FUNCTIONS[name] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == [ctypes.c_void_p, ctypes.c_void_p]
    assert _lib.FUNCTIONS[H_SIZE] == (ctypes.c_size_t, [ctypes.c_void_p])
    assert lib.nfi_version() >= 107
    # the header comments cite the reference lines the entries replace
    comment = open(_lib.HEADER).read().split('typedef struct nfi_synth_head_args')[0].rsplit('/*', 1)[1]
    for cited in ('stylegan.py:325-356', '372-380', '173-177', '127-130', '132', '373'):
        assert cited in comment, cited
    assert 'stylegan.py:132' in open(_lib.HEADER).read().split('typedef struct nfi_synth_modulate_args')[0].rsplit('/*', 1)[1]


def test_struct_field_order():
    assert [n for n, _ in _lib.STRUCT_FIELDS[HEAD]] == [
        'batch', 'latent_dim', 'in_channels', 'out_channels', 'taps', 'latent_stride', 'demodulate', 'weight_gain', 'bias_gain', 'style_gain',
        'latent', 'affine_weight', 'affine_bias', 'weight', 'styles', 'dcoefs', 'g_styles', 'g_dcoefs', 'g_latent', 'g_affine_weight',
        'g_affine_bias', 'g_weight', 'workspace', 'workspace_bytes']
    kinds = dict(_lib.STRUCT_FIELDS[HEAD])
    assert all(kinds[k] is ctypes.c_float for k in ('weight_gain', 'bias_gain', 'style_gain')) and kinds['workspace_bytes'] is ctypes.c_size_t
    assert all(kinds[k] is ctypes.c_int for k in ('batch', 'latent_dim', 'in_channels', 'out_channels', 'taps', 'latent_stride', 'demodulate'))
    assert [n for n, _ in _lib.STRUCT_FIELDS[MOD]] == ['batch', 'channels', 'plane', 'x', 'styles', 'out', 'g_out', 'g_x', 'g_styles']


HEAD_BASE = dict(batch=2, latent_dim=8, in_channels=5, out_channels=20, taps=9, latent_stride=8, demodulate=1, weight_gain=0.35, bias_gain=1.0,
                 style_gain=1.0, latent=16, affine_weight=16, affine_bias=16, weight=16, styles=16, dcoefs=16, g_styles=16, g_dcoefs=16,
                 g_latent=16, g_affine_weight=None, g_affine_bias=None, g_weight=None, workspace=16, workspace_bytes=1 << 20)


def refused(lib, struct, base, word, entries, **kw):
    a = _lib.make_args(struct, **dict(base, **kw))
    for entry in entries:
        rc, msg = getattr(lib, entry)(ctypes.byref(a), None), lib.nfi_last_error()
        assert rc == -1 and word in msg, (entry, kw, word, rc, msg)


def test_head_refusals_come_with_the_argument_named_and_before_any_launch(lib):
    """Every pointer here is the number 16: a launch would fault, a refusal never reads it."""
    both = (H_FWD, H_BWD)
    no = functools.partial(refused, lib, HEAD, HEAD_BASE)
    for entry in both:
        assert getattr(lib, entry)(None, None) == -1 and b'null argument struct' in lib.nfi_last_error()
    for field in ('latent', 'affine_weight', 'styles'):
        no(b'null %s' % field.encode(), both, **{field: None})
        assert lib.nfi_last_error().endswith(b'null %s' % field.encode())               # that argument and no other
    for size in (dict(batch=0), dict(latent_dim=0, latent_stride=0), dict(in_channels=0), dict(out_channels=0), dict(taps=0), dict(batch=-3),
                 dict(taps=-1)):
        no(b'must be at least 1', both, **size)
    for stride in (7, 0, -8):
        no(b'latent_stride', both, latent_stride=stride)
    no(b'demodulate without weight', both, weight=None)
    no(b'demodulate without dcoefs', both, dcoefs=None)
    for gain in ('weight_gain', 'bias_gain', 'style_gain'):
        no(gain.encode(), both, **{gain: float('nan')})
    # element counts: 2^16 x 2^15 affine weights; 2^11 x 2^11 x 2^9 convolution weights; rows 2^20 apart for 2^11 images;
    # more than 8 x 65535 images or rows (the launches' second grid dimension)
    no(b'element count', both, in_channels=1 << 16, latent_dim=1 << 15, latent_stride=1 << 15)
    no(b'element count', both, in_channels=1 << 11, out_channels=1 << 11, taps=1 << 9)
    no(b'element count', both, batch=1 << 11, latent_stride=1 << 20)
    no(b'element count', both, batch=8 * 65535 + 1, in_channels=1, out_channels=1, latent_dim=1, latent_stride=1)
    no(b'element count', both, out_channels=8 * 65535 + 1, in_channels=1, taps=1)
    # the backward
    no(b'no upstream gradient', (H_BWD,), g_styles=None, g_dcoefs=None)
    no(b'no gradient asked for', (H_BWD,), g_latent=None)
    no(b'g_dcoefs without dcoefs', (H_BWD,), demodulate=0, dcoefs=None)
    no(b'g_dcoefs without dcoefs', (H_BWD,), demodulate=0)
    no(b'g_weight without g_dcoefs', (H_BWD,), g_weight=16, g_dcoefs=None)
    # the workspace, float64: g_s [B,I], ceil(I / 16) shares of g_latent [B,D] and, with demodulate, ceil(O / 8) shares of t [B,I]
    n_ws = _lib.struct_query(H_SIZE, HEAD, batch=2, latent_dim=8, in_channels=5, out_channels=20, taps=9, demodulate=1)
    assert n_ws == ((3 + 1) * 2 * 5 + 1 * 2 * 8) * 8
    assert _lib.struct_query(H_SIZE, HEAD, batch=2, latent_dim=8, in_channels=5, out_channels=20, taps=9, demodulate=0) == (2 * 5 + 2 * 8) * 8
    assert _lib.struct_query(H_SIZE, HEAD, batch=2, latent_dim=8, in_channels=33, out_channels=20, taps=9, demodulate=0) == (2 * 33 + 3 * 2 * 8) * 8
    no(b'workspace missing', (H_BWD,), workspace=None)
    no(b'workspace missing or not 8-byte aligned', (H_BWD,), workspace=12)
    no(b'workspace too small', (H_BWD,), workspace_bytes=n_ws - 1)
    with pytest.raises(RuntimeError, match='style_gain'):
        _lib.call_struct(H_FWD, HEAD, 0, **dict(HEAD_BASE, style_gain=float('nan')))


def test_the_workspace_query_returns_zero_for_refused_shapes(lib):
    assert lib.nfi_synth_head_bwd_workspace_bytes(None) == 0
    ok = dict(batch=2, latent_dim=8, in_channels=5, out_channels=20, taps=9, demodulate=1)
    assert _lib.struct_query(H_SIZE, HEAD, **ok) > 0
    for bad in (dict(batch=0), dict(latent_dim=0), dict(in_channels=-1), dict(out_channels=0), dict(taps=0),
                dict(in_channels=1 << 16, latent_dim=1 << 15), dict(in_channels=1 << 11, out_channels=1 << 11, taps=1 << 9),
                dict(batch=8 * 65535 + 1, in_channels=1, out_channels=1, latent_dim=1)):
        assert _lib.struct_query(H_SIZE, HEAD, **dict(ok, **bad)) == 0, bad


def test_modulate_refusals_come_with_the_argument_named_and_before_any_launch(lib):
    base = dict(batch=2, channels=3, plane=16, x=16, styles=16, out=16, g_out=16, g_x=16, g_styles=None)
    no = functools.partial(refused, lib, MOD, base)
    both = (M_FWD, M_BWD)
    for entry in both:
        assert getattr(lib, entry)(None, None) == -1 and b'null argument struct' in lib.nfi_last_error()
    no(b'null styles', both, styles=None)
    no(b'null x', (M_FWD,), x=None)
    no(b'null out', (M_FWD,), out=None)
    no(b'null g_out', (M_BWD,), g_out=None)
    no(b'no gradient asked for', (M_BWD,), g_x=None)
    no(b'g_styles without x', (M_BWD,), g_styles=16, x=None)
    for size in (dict(batch=0), dict(channels=0), dict(plane=0), dict(plane=-16)):
        no(b'must be at least 1', both, **size)
    no(b'element count', both, batch=1 << 5, channels=1 << 10, plane=1 << 16)              # 2^31 elements
    with pytest.raises(RuntimeError, match='plane'):
        _lib.call_struct(M_FWD, MOD, 0, **dict(base, plane=0))


def test_no_cpu_path(monkeypatch):
    """A host tensor is refused before the library is reached, by the wrappers and by the nodes.  (The wrappers check the
    device first, so their refusals of a wrong dtype, element count or second device need device tensors: they are in
    tests/test_synth_head_gpu.py.)"""
    from nerf_from_image_amd import ops, synthesis
    monkeypatch.setattr(_lib, 'call_struct', lambda *a, **k: pytest.fail('reached the library'))
    t = hu.make_head_inputs(2, 8, 5, 3, 9)
    lin = torch.nn.Linear(8, 5)
    lin.weight_gain, lin.bias_gain = t['weight_gain'], 1.0
    x, s = torch.randn(2, 5, 4, 4), torch.randn(2, 5)
    for call in (lambda: ops.synth_head(t['latent'], t['A'], t['a_bias'], t['weight_gain'], 1.0, t['W']),
                 lambda: ops.synth_head_bwd(t['g_styles'], t['g_dcoefs'], t['g_styles'], t['g_dcoefs'], t['latent'], t['A'], t['a_bias'],
                                            t['weight_gain'], 1.0, t['W']),
                 lambda: ops.synth_modulate(x, s), lambda: ops.synth_modulate_bwd(x, x, s),
                 lambda: synthesis.layer_styles(t['latent'], lin, t['W']), lambda: synthesis.modulate(x, s)):
        with pytest.raises(RuntimeError, match='GPU'):
            call()


def test_attach_has_the_option_off_by_default_and_documented_next_to_the_tail():
    from nerf_from_image_amd import generator
    params = inspect.signature(generator.attach).parameters
    assert params['fused_synthesis_head'].default is False and params['fused_synthesis_tail'].default is False
    assert list(params)[-2:] == ['fused_synthesis_head', 'fused_synthesis_tail']
    doc = generator.attach.__doc__
    assert doc.index('fused_synthesis_tail (off by default)') < doc.index('fused_synthesis_head (off by default') < doc.index('hip_regularisers:')
    src = inspect.getsource(generator)
    assert src.count('synthesis.unfused(self.synthesis_network)') == 2          # both forwards that serve path_length


@needs_reference
def test_fuse_with_the_head_swaps_every_layer_and_output_layer_and_leaves_the_state_dict_alone():
    from nerf_from_image_amd import handoff, synthesis
    stylegan = reference.modules().stylegan
    net, _, _ = hu.small_network(stylegan)
    keys, values = list(net.state_dict().keys()), [v.clone() for v in net.state_dict().values()]
    layers = [m for m in net.modules() if isinstance(m, stylegan.SynthesisLayer)]
    outs = [m for m in net.modules() if isinstance(m, stylegan.OutputLayer)]
    assert len(layers) == 5 and len(outs) == 3
    assert synthesis.output_layers(net) == outs and synthesis.synthesis_layers(net) == layers      # by attribute: exactly the classes' instances
    originals = [m.forward for m in layers + outs]
    # head=False is today's behaviour: the output layers keep their forward, the layers' flag is off
    assert synthesis.fuse_layers(net) == layers and synthesis.fused_output_layers(net) == [] and not synthesis.head_fused(net)
    assert all('forward' not in m.__dict__ for m in outs) and all(m._nfi_fused_head is False for m in layers)
    assert synthesis.fuse_layers(net, head=True) == layers and synthesis.fused_layers(net) == layers
    assert synthesis.fused_output_layers(net) == outs and synthesis.head_fused(net)
    synthesis.fuse_layers(net, head=True)                                        # again: nothing nests
    for m in layers:
        assert m.forward.__func__ is synthesis.fused_layer_forward and m._nfi_fused_head is True
        assert m._nfi_original_forward.__func__ is stylegan.SynthesisLayer.forward
    for m in outs:
        assert m.forward.__func__ is synthesis.fused_output_forward and m.forward.__self__ is m
        assert m._nfi_original_forward.__func__ is stylegan.OutputLayer.forward
    with synthesis.unfused(net):
        assert [m.forward for m in layers + outs] == originals
        assert net(torch.randn(2, net.num_ws, 32), noise_mode='const').shape == (2, 96, 16, 16)      # the reference's own ops, on the CPU
    assert all(m.forward.__func__ is synthesis.fused_output_forward for m in outs)
    with pytest.raises(RuntimeError, match='GPU'):                               # fused: no CPU path
        net(torch.randn(2, net.num_ws, 32), noise_mode='const')
    # the hand-off's fused last block takes its toRGB styles from the head node: no CPU path there either
    blk = handoff.fuse_last_block(net)
    assert blk.torgb in outs and blk.torgb._nfi_fused_head is True
    handoff.unfuse_last_block(net)
    # head=False on a network fused with the head: the output layers get their forward back, the layers stay fused
    synthesis.fuse_layers(net)
    assert synthesis.fused_output_layers(net) == [] and synthesis.fused_layers(net) == layers and not synthesis.head_fused(net)
    assert all(not hasattr(m, '_nfi_fused_head') and 'forward' not in m.__dict__ or m.forward == o for m, o in zip(outs, originals[5:]))
    synthesis.fuse_layers(net, head=True)
    assert synthesis.unfuse_layers(net) == layers and synthesis.fused_layers(net) == [] and synthesis.fused_output_layers(net) == []
    assert all('forward' not in m.__dict__ or m.forward == o for m, o in zip(layers + outs, originals))
    assert all(not hasattr(m, '_nfi_original_forward') and not hasattr(m, '_nfi_fused_head') for m in layers + outs)
    assert list(net.state_dict().keys()) == keys
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), values))


@needs_reference
def test_the_restated_styles_are_the_live_affine():
    """layer.affine(w), float32 on the CPU, against the float32 restatement: the same operations, the same bits; and within
    float32 rounding of a 24-term sum of the float64 one (24 x 2^-24 of the largest |styles|, a loose bound on both sides'
    rounding)."""
    stylegan = reference.modules().stylegan
    torch.manual_seed(2)
    for layer, gain in ((stylegan.SynthesisLayer(6, 5, w_dim=24, resolution=8), 1.0), (stylegan.OutputLayer(6, 5, w_dim=24), None)):
        with torch.no_grad():
            layer.affine.bias.normal_()
            w = torch.randn(3, 24)
            theirs = layer.affine(w) if gain is not None else layer.affine(w) * layer.weight_gain
            a = layer.affine
            sg = 1.0 if gain is not None else layer.weight_gain
            ours, _ = hu.head_ref(w, a.weight, a.bias, a.weight_gain, a.bias_gain, layer.weight, False, sg, torch.float32)
            ours64, _ = hu.head_ref(w, a.weight, a.bias, a.weight_gain, a.bias_gain, layer.weight, False, sg)
        assert torch.equal(theirs, ours)
        assert float((theirs.double() - ours64).abs().max()) <= 24 * 2.0 ** -24 * float(ours64.abs().max())


@needs_reference
@pytest.mark.parametrize('kind', ['plain', 'up', 'output'])
def test_the_restatement_is_the_live_layer(kind):
    """SynthesisLayer.forward (`up` and plain) and OutputLayer.forward of the live reference in float64 on the CPU, against
    the restated head, the reference's own convolution call and synth_tail_util.tail_ref, all in float64: the same
    expressions, so they agree to float64 rounding - 1e-12 of the output's largest magnitude leaves four orders of room
    over 2^-53 x the few hundred operations per element."""
    stylegan = reference.modules().stylegan
    torch.manual_seed(3)
    up = kind == 'up'
    if kind == 'output':
        layer = stylegan.OutputLayer(6, 5, w_dim=8).double()
    else:
        layer = stylegan.SynthesisLayer(6, 5, w_dim=8, resolution=12, up=up).double()
        with torch.no_grad():
            layer.noise_strength.fill_(0.7)
    with torch.no_grad():
        layer.bias.normal_()
        layer.affine.bias.normal_()
    side = 6 if up else 12
    x, w = torch.randn(3, 6, side, side, dtype=torch.float64), torch.randn(3, 8, dtype=torch.float64)
    a = layer.affine
    with torch.no_grad():
        if kind == 'output':
            theirs = layer(x, w)
            styles, none = hu.head_ref(w, a.weight, a.bias, a.weight_gain, a.bias_gain, layer.weight, False, layer.weight_gain)
            assert none is None
            ours = F.conv2d(hu.modulate_ref(x, styles), layer.weight) + layer.bias.view(1, -1, 1, 1)
        else:
            theirs = layer(x, w, noise_mode='const', gain=0.75)
            styles, dcoefs = hu.head_ref(w, a.weight, a.bias, a.weight_gain, a.bias_gain, layer.weight, True, 1.0)
            xs = hu.modulate_ref(x, styles)
            y = F.conv_transpose2d(xs, layer.weight.transpose(0, 1), stride=2) if up else F.conv2d(xs, layer.weight, padding=1)
            ours = su.tail_ref(y, dcoefs, layer.noise_const * layer.noise_strength, layer.bias, layer.resample_filter, layer.act_gain * 0.75,
                               up, True)
    assert ours.dtype == theirs.dtype == torch.float64 and ours.shape == theirs.shape
    err, scale = float((theirs - ours).abs().max()), float(theirs.abs().max())
    print('live %s layer against the restatement in float64: %.3e, scale %.3g' % (kind, err, scale))
    assert err <= 1e-12 * scale


@pytest.mark.parametrize('name', ['one', 'wave_and_tail', 'odd_row', 'largest'])
def test_the_factored_demodulation_is_the_reference_expression_in_float64(name):
    """sum_{i,k} (W s)^2 = sum_i s^2 Q[o,i] in float64: the two differ by the order of I K additions of positive terms,
    at most I K x 2^-53 relative, halved by the rsqrt; 2^-40 is loose for I K = 4608.  The float32 factored form stays as
    close to float64 as the reference's float32 expression does (a factor 4 and the 2^-21 floor of the GPU tests allow for
    the scatter between two roundings of the same quantity)."""
    B, D, I, O, K, demod, sg = hu.HEAD_SHAPES[name]
    c = hu.head_case(B, D, I, O, K, demod, sg)
    t = c['inputs']
    styles, dcoefs = c['want']['styles'], c['want']['dcoefs']
    got = hu.dcoefs_factored(styles, t['W'].double())
    rel = float(((got - dcoefs) / dcoefs).abs().max())
    own32 = float((hu.dcoefs_factored(styles.float(), t['W']).double() - dcoefs).abs().max())
    print('factored demodulation %s: float64 relative %.3e; float32 factored %.3e, float32 reference %.3e' % (name, rel, own32, c['e32']['dcoefs']))
    assert rel <= 2.0 ** -40
    assert own32 <= max(4 * c['e32']['dcoefs'], hu.FLOOR * max(1.0, float(dcoefs.abs().max())))
