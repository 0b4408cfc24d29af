"""CPU-side checks of the synthesis-layer tail (csrc/nfi_synth_tail.inc, nerf_from_image_amd/synthesis.py): the entries are
exported with the header's prototypes and refuse what the header says they refuse - with the argument named, before any
launch; layer_tail has no CPU path; attach has the option, off; fuse_layers / unfuse_layers / unfused swap and restore the
forward of every layer of the LIVE reference SynthesisNetwork and leave its state_dict alone; and the tests' own yardstick
(tests/synth_tail_util.py) is the live SynthesisLayer.forward, can tell each deliberately broken variant from the truth,
and excludes the share of near-kink elements it says it does."""
import ctypes
import inspect
import math
import re

import pytest
import torch
import torch.nn.functional as F

from nerf_from_image_amd import _lib
from oracle import reference
import synth_tail_util as su

needs_reference = pytest.mark.skipif(not reference.available(), reason='reference sources not available (oracle/make_ref.py)')
STRUCT, FWD, BWD, SIZE = 'nfi_synth_tail_args', 'nfi_synth_tail_fwd', 'nfi_synth_tail_bwd', 'nfi_synth_tail_bwd_workspace_bytes'


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    return _lib.load()


def test_entries_are_exported_with_the_header_prototypes(lib):
    src = _lib._strip_comments(open(_lib.HEADER).read())
    found = {m.group(2): (m.group(1), [p.strip() for p in m.group(3).split(',')])
             for m in re.finditer(r'(\w+)\s+(nfi_synth_tail\w*)\s*\(([^)]*)\)\s*;', src)}
    two = ['const %s* a' % STRUCT, 'nfi_stream_t stream']
    assert found == {FWD: ('int', two), BWD: ('int', two), SIZE: ('size_t', ['const %s* a' % STRUCT])}
    for name in (FWD, BWD):
        assert _lib.FUNCTIONS[name] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == [ctypes.c_void_p, ctypes.c_void_p]
    assert _lib.FUNCTIONS[SIZE] == (ctypes.c_size_t, [ctypes.c_void_p])
    assert lib.nfi_version() >= 106
    # the header comment cites the reference lines the entries replace
    comment = open(_lib.HEADER).read().split('typedef struct nfi_synth_tail_args')[0].rsplit('/*', 1)[1]
    for cited in ('stylegan.py:325-356', '101-105', '139-140', '351'):
        assert cited in comment, cited


def test_struct_field_order():
    assert [n for n, _ in _lib.STRUCT_FIELDS[STRUCT]] == [
        'batch', 'channels', 'resolution', 'in_size', 'up', 'activate', 'act_gain', 'slope', 'y', 'dcoefs', 'bias', 'taps', 'noise',
        'noise_shared', 'out', 'g_out', 'g_y', 'g_dcoefs', 'g_bias', 'g_noise', 'workspace', 'workspace_bytes']
    kinds = dict(_lib.STRUCT_FIELDS[STRUCT])
    assert kinds['act_gain'] is ctypes.c_float and kinds['slope'] is ctypes.c_float and kinds['workspace_bytes'] is ctypes.c_size_t
    assert all(kinds[k] is ctypes.c_void_p for k in ('y', 'dcoefs', 'bias', 'taps', 'noise', 'out', 'g_out', 'g_y', 'g_dcoefs', 'g_bias',
                                                     'g_noise', 'workspace'))


def test_refusals_come_with_the_argument_named_and_before_any_launch(lib):
    """Every pointer here is the number 16: a launch would fault, a refusal never reads it."""
    base = dict(batch=2, channels=3, resolution=8, in_size=9, up=1, activate=1, act_gain=math.sqrt(2.0), slope=0.2, y=16, dcoefs=16,
                bias=16, taps=16, noise=None, noise_shared=0, out=16, g_out=16, g_y=16, g_dcoefs=None, g_bias=None, g_noise=None,
                workspace=None, workspace_bytes=0)

    def refused(word, entries=(FWD, BWD), **kw):
        a = _lib.make_args(STRUCT, **dict(base, **kw))
        for entry in entries:
            rc, msg = getattr(lib, entry)(ctypes.byref(a), None), lib.nfi_last_error()
            assert rc == -1 and word in msg, (entry, kw, word, rc, msg)

    for entry in (FWD, BWD):
        assert getattr(lib, entry)(None, None) == -1 and b'null argument struct' in lib.nfi_last_error()
    for field in ('y', 'dcoefs', 'bias', 'out'):
        refused(b'null %s' % field.encode(), **{field: None})
        assert lib.nfi_last_error().endswith(b'null %s' % field.encode())               # that argument and no other
    refused(b'taps', taps=None)
    refused(b'g_out', entries=(BWD,), g_out=None)
    refused(b'no gradient asked for', entries=(BWD,), g_y=None)
    for in_size in (8, 10, 0, -1):                                  # up: the input side must be R + 1
        refused(b'in_size', in_size=in_size)
    for in_size in (9, 7):                                          # without up: R itself
        refused(b'in_size', up=0, in_size=in_size)
    for size in (dict(batch=0), dict(channels=0), dict(resolution=0, in_size=1), dict(batch=-1), dict(resolution=-4, in_size=-3)):
        refused(b'batch, channels and resolution', **size)
    refused(b'resolution must be at most', resolution=16385, in_size=16386)
    for gain in (0.0, -1.0, float('nan')):
        refused(b'act_gain', act_gain=gain)
    for slope in (-0.2, float('nan')):
        refused(b'slope', slope=slope)
    # ceil(16384 / 64)^2 = 2^16 tiles per plane: 2^15 planes reach the launch limit
    refused(b'element count', batch=1 << 8, channels=1 << 7, resolution=16384, in_size=16385)
    refused(b'element count', up=0, batch=1 << 10, channels=1 << 5, resolution=16384, in_size=16384)      # 2^16 chunks per plane
    assert lib.nfi_synth_tail_bwd_workspace_bytes(None) == 0
    assert _lib.struct_query(SIZE, STRUCT, batch=1 << 8, channels=1 << 7, resolution=16384, up=1) == 0
    # the sums need their workspace: one float64 pair per block, ceil(9 / 64)^2 = 1 block per plane here
    n_ws = _lib.struct_query(SIZE, STRUCT, batch=2, channels=3, resolution=8, up=1)
    assert n_ws == 2 * 3 * 1 * 2 * 8
    assert _lib.struct_query(SIZE, STRUCT, batch=2, channels=3, resolution=64, up=1) == 2 * 3 * 4 * 2 * 8      # 65 -> 2 x 2 tiles
    assert _lib.struct_query(SIZE, STRUCT, batch=2, channels=3, resolution=65, up=0) == 2 * 3 * 2 * 2 * 8      # 4225 -> 2 chunks
    refused(b'workspace', entries=(BWD,), g_bias=16)
    refused(b'workspace', entries=(BWD,), g_dcoefs=16, workspace=12, workspace_bytes=n_ws)
    refused(b'workspace too small', entries=(BWD,), g_dcoefs=16, workspace=16, workspace_bytes=n_ws - 1)
    with pytest.raises(RuntimeError, match='act_gain'):
        _lib.call_struct(FWD, STRUCT, 0, **dict(base, act_gain=0.0))


def test_no_cpu_path():
    from nerf_from_image_amd import ops, synthesis
    t = su.make_inputs(1, 2, 4, True, 'batch')
    for call in (lambda: synthesis.layer_tail(t['y'], t['dcoefs'], t['noise'], t['bias'], t['taps'], su.ACT_GAIN, True),
                 lambda: synthesis.layer_tail(t['y'], t['dcoefs'], None, t['bias'], t['taps'], su.ACT_GAIN, True),
                 lambda: ops.synth_tail(t['y'], t['dcoefs'], t['noise'], t['bias'], t['taps'], su.ACT_GAIN, True),
                 lambda: ops.synth_tail_bwd(t['g_out'], t['g_out'], t['y'], t['dcoefs'], t['noise'], t['bias'], t['taps'], su.ACT_GAIN, True)):
        with pytest.raises(RuntimeError, match='GPU'):
            call()


def test_attach_has_the_option_off_by_default():
    from nerf_from_image_amd import generator
    params = inspect.signature(generator.attach).parameters
    assert list(params)[-1] == 'fused_synthesis_tail' and params['fused_synthesis_tail'].default is False
    src = inspect.getsource(generator)
    assert src.count('synthesis.unfused(self.synthesis_network)') == 2          # both forwards that serve path_length


def small_network(stylegan, seed=0):
    torch.manual_seed(seed)
    net = stylegan.SynthesisNetwork(w_dim=32, img_resolution=16, img_channels=96, channel_max=16)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith('noise_strength'):
                p.fill_(0.3)
            elif name.endswith('bias'):
                p.normal_()
    return net


@needs_reference
def test_fuse_unfuse_and_unfused_swap_every_layer_and_leave_the_state_dict_alone():
    from nerf_from_image_amd import handoff, synthesis
    stylegan = reference.modules().stylegan
    net = small_network(stylegan)
    keys, values = list(net.state_dict().keys()), [v.clone() for v in net.state_dict().values()]
    layers = [m for m in net.modules() if isinstance(m, stylegan.SynthesisLayer)]
    assert len(layers) == 5 and synthesis.synthesis_layers(net) == layers        # found by attribute: exactly the class's instances
    assert synthesis.fused_layers(net) == []
    originals = [m.forward for m in layers]
    assert synthesis.fuse_layers(net) == layers and synthesis.fused_layers(net) == layers
    for m in layers:
        assert m.forward.__func__ is synthesis.fused_layer_forward and m.forward.__self__ is m
    synthesis.fuse_layers(net)                                                   # again: nothing nests
    assert all(m._nfi_original_forward.__func__ is stylegan.SynthesisLayer.forward for m in layers)
    with synthesis.unfused(net):
        assert [m.forward for m in layers] == originals
        ws = torch.randn(2, net.num_ws, 32)
        assert net(ws, noise_mode='const').shape == (2, 96, 16, 16)               # the reference's own ops, on the CPU
    assert all(m.forward.__func__ is synthesis.fused_layer_forward for m in layers)
    with pytest.raises(RuntimeError, match='GPU'):                               # fused: no CPU path
        net(torch.randn(2, net.num_ws, 32), noise_mode='const')
    # composes with the hand-off's swap of the last block, in either order of undoing
    blk = handoff.fuse_last_block(net)
    assert blk.conv0 in layers and blk.conv1 in layers and synthesis.fused_layers(net) == layers
    handoff.unfuse_last_block(net)
    assert synthesis.unfuse_layers(net) == layers and synthesis.fused_layers(net) == []
    assert all('forward' not in m.__dict__ or m.forward == o for m, o in zip(layers, originals))
    assert all(not hasattr(m, '_nfi_original_forward') for m in layers)
    assert list(net.state_dict().keys()) == keys
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), values))
    with pytest.raises(AttributeError, match='synthesis layer'):
        synthesis.fuse_layers(torch.nn.Sequential(torch.nn.Linear(3, 3)))
    with synthesis.unfused(torch.nn.Linear(3, 3)):                               # nothing to do, nothing raised
        pass


@needs_reference
@pytest.mark.parametrize('up', [False, True])
@pytest.mark.parametrize('noise_mode', ['const', 'random'])
def test_the_restatement_is_the_live_layer_tail(up, noise_mode):
    """SynthesisLayer.forward of the live reference, float32 on the CPU, against its own convolution followed by the float32
    restatement: within float32 rounding - the two differ by the filter's summation order and the fusing of addcmul, at most
    16 + 6 roundings of 2^-24 of the scale each, 1.3e-6; the bound is 2e-6 of the output's largest magnitude."""
    stylegan = reference.modules().stylegan
    torch.manual_seed(3)
    layer = stylegan.SynthesisLayer(6, 5, w_dim=8, resolution=12, up=up)
    with torch.no_grad():
        layer.bias.normal_()
        layer.noise_strength.fill_(0.7)
    x, w = torch.randn(3, 6, 6 if up else 12, 6 if up else 12), torch.randn(3, 8)
    with torch.no_grad():
        torch.manual_seed(5)
        theirs = layer(x, w, noise_mode=noise_mode, gain=0.75)
        torch.manual_seed(5)
        styles = layer.affine(w)
        noise = (torch.randn(3, 1, 12, 12) if noise_mode == 'random' else layer.noise_const) * layer.noise_strength
        dcoefs = ((layer.weight.unsqueeze(0) * styles.reshape(3, 1, -1, 1, 1)).square().sum(dim=[2, 3, 4]) + 1e-8).rsqrt()
        xs = x * styles.reshape(3, -1, 1, 1)
        y = F.conv_transpose2d(xs, layer.weight.transpose(0, 1), stride=2) if up else F.conv2d(xs, layer.weight, padding=1)
        ours = su.tail_ref(y, dcoefs, noise, layer.bias, layer.resample_filter, layer.act_gain * 0.75, up, True, dtype=torch.float32)
        ours64 = su.tail_ref(y, dcoefs, noise, layer.bias, layer.resample_filter, layer.act_gain * 0.75, up, True)
    assert ours.dtype == torch.float32 and ours.shape == theirs.shape == (3, 5, 12, 12)
    scale = float(theirs.abs().max())
    err, err64 = float((theirs - ours).abs().max()), float((theirs.double() - ours64).abs().max())
    print('live layer tail against the restatement (up=%s, %s): float32 %.3e, float64 %.3e, scale %.3g' % (up, noise_mode, err, err64, scale))
    assert err <= 2e-6 * scale and err64 <= 2e-6 * scale


CPU_CASES = [(3, 16, 16, False, 'batch'), (3, 16, 24, True, 'batch'), (2, 5, 64, True, 'shared'), (2, 5, 5, False, 'shared')]


@pytest.mark.parametrize('variant', su.VARIANTS)
def test_the_bound_tells_each_broken_variant_from_the_truth(variant):
    """Each deliberately broken restatement misses the float64 yardstick by more than 100 x the parity tolerance of its case."""
    for B, C, R, up, noise_kind in CPU_CASES:
        if variant in ('shifted', 'no_padding', 'no_gain') and not up:
            continue
        for taps_kind in su.TAPS:
            c = su.case(B, C, R, up, noise_kind, True, taps_kind)
            t = c['inputs']
            broken = su.tail_ref(t['y'], t['dcoefs'], t['noise'], t['bias'], t['taps'], c['gain'], up, True, variant=variant)
            miss, tol = float((broken - c['out']).abs().max()), su.tolerance(c['e32']['out'])
            assert tol <= 1e-5, tol                                             # the bound itself stays at float32 rounding
            assert miss > 100 * tol, (variant, (B, C, R, up), taps_kind, miss, tol)


def test_the_excluded_share_is_what_the_normal_density_says():
    """|pre64| < 1e-3 std: about 2 phi(0) 1e-3 = 0.08 % of the elements, never over 0.5 % in a case; with activate off none."""
    shares = []
    for B, C, R, up, noise_kind in CPU_CASES:
        c = su.case(B, C, R, up, noise_kind, True)
        assert c['excluded'] <= 0.005, ((B, C, R, up), c['excluded'])
        assert bool((c['g_out'][c['near']] == 0).all()) and bool((c['g_out'][~c['near']] == c['inputs']['g_out'][~c['near']]).all())
        shares.append((c['near'].sum().item(), c['near'].numel()))
        assert su.case(B, C, R, up, noise_kind, False)['excluded'] == 0.0
    share = sum(n for n, _ in shares) / sum(n for _, n in shares)
    print('excluded share over %d elements: %.4f %%' % (sum(n for _, n in shares), 100 * share))
    assert 0.0002 <= share <= 0.002
