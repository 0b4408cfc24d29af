"""The regulariser's ordered backward on the GPU: nfi_sdf_gradient_bwd_ordered (ops.sdf_gradient_bwd(..., ordered=True))
and the branch of a model attached with deterministic_backward=True return the same bits on every launch - and the right
gradients: test_regulariser_operator.py's cases against its float64 oracle at that file's bounds, and against the atomic
entry at its "same sum, other order" bound."""
import copy
import hashlib

import pytest
import torch

from parity_util import grad_close
from nerf_from_image_amd import _lib, ops
from oracle import nfi_oracle as orc
from stand_in import StandInGenerator
import nerf_from_image_amd.generator as nfi_gen
from test_regulariser_operator import CASE, PARAMS, reference, texels_of, check_backward, range_of

pytestmark = pytest.mark.gpu

# two_chunks_per_wave: 16 x 5003 points on 8^2 cells: runs of ~78 entries per cell (more than one 32-entry block of the
# gather), waves that carry two chunks into one slot; res257: cell indices need a third radix pass; nodes: points whose
# cell the keys and the kernel must agree on
NAMES = ['base', 'one_point_res2', 'tail_P63', 'tail_P64', 'tail_P65', 'two_chunks_per_wave', 'upstream_per_point', 'res257',
         'lattice_res385', 'nodes']
LAUNCHES = [(n, False) for n in NAMES] + [('base', True)]
LAUNCH_IDS = [n + ('-interleaved' if i else '') for n, i in LAUNCHES]
KEYS = ('g_texels', 'g_w1', 'g_b1', 'g_w2', 'g_b2')


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def raw_bwd(name, texels, ordered, g_sdf='u_d', g_gradient='u_g'):
    """ops.sdf_gradient_bwd's own dict; g_sdf / g_gradient: a key of the case's inputs, a tensor, or None (a NULL pointer)."""
    c, t, dev = CASE[name], reference(name)[0], texels.device
    up = lambda v: None if v is None else (t[v] if isinstance(v, str) else v).to(dev)
    return ops.sdf_gradient_bwd(t['x'].to(dev), texels, t['w1'].to(dev), t['b1'].to(dev), t['w2'].to(dev), t['b2'].to(dev), range_of(c),
                                up(g_sdf), up(g_gradient), ordered=ordered)


def by_param(out):
    return {'planes': ops.texel_grad_to_planes(out['g_texels']), 'w1': out['g_w1'], 'b1': out['g_b1'], 'w2': out['g_w2'], 'b2': out['g_b2']}


@pytest.mark.parametrize('name,interleaved', LAUNCHES, ids=LAUNCH_IDS)
def test_ordered_backward_case(gpu_device, name, interleaved):
    """Six launches give one sha256 per output; the first is held to the float64 oracle at check_backward's bounds
    (max(5e-4, 4 x the float32 oracle's distance)) and to the atomic entry within 2e-5 of that output's largest entry;
    rows 1.. of a 33-row second layer stay exactly zero.  (That the atomic entry differs from launch to launch is not
    asserted: nothing guarantees it.)"""
    c = CASE[name]
    t, r64, r32 = reference(name)
    texels = texels_of(t, gpu_device, interleaved)
    first = raw_bwd(name, texels, True)
    assert float(first['g_texels'].abs().max()) > 0 and float(first['g_w1'].abs().max()) > 0
    want = {k: sha(first[k]) for k in KEYS}
    for launch in range(1, 6):
        again = raw_bwd(name, texels, True)
        assert {k: sha(again[k]) for k in KEYS} == want, (name, launch, [k for k in KEYS if not torch.equal(again[k], first[k])])
    what = 'ordered ' + name + (' (interleaved)' if interleaved else '')
    got = by_param(first)
    check_backward(what, got, r64, r32)
    if c.n_out == 33:
        assert not got['w2'][1:].any() and not got['b2'][1:].any(), what
    atomic = by_param(raw_bwd(name, texels, False))
    for k in PARAMS:
        grad_close(got[k], atomic[k], 2e-5, '%s vs atomic entry: grad %s' % (what, k))


def test_null_upstream_gradients(gpu_device):
    """g_gradient == NULL equals the launch with an all-zero g_gradient bit for bit in this mode, and matches the oracle
    with that term left out of the loss; likewise g_sdf == NULL; both NULL is refused with a message."""
    t = reference('base')[0]
    texels = texels_of(t, gpu_device)
    for null, kw_null, kw_zero, ref_kw in (
            ('g_gradient', dict(g_gradient=None), dict(g_gradient=torch.zeros_like(t['u_g'])), dict(use_g=False)),
            ('g_sdf', dict(g_sdf=None), dict(g_sdf=torch.zeros_like(t['u_d'])), dict(use_d=False))):
        got, zero = raw_bwd('base', texels, True, **kw_null), raw_bwd('base', texels, True, **kw_zero)
        for k in KEYS:
            assert torch.equal(got[k], zero[k]), (null, k)
        _, r64, r32 = reference('base', **ref_kw)
        check_backward('ordered, %s = NULL' % null, by_param(got), r64, r32)
    with pytest.raises(RuntimeError, match='no upstream gradient'):
        raw_bwd('base', texels, True, g_sdf=None, g_gradient=None)


def test_backward_accumulates_into_its_outputs(gpu_device):
    """The ABI's contract, through the raw entry and with a workspace full of 0xFF bytes (nothing in it may need the
    caller's zeroing): after one launch each output holds its O(1) random pre-fill (drawn as
    test_regulariser_operator.test_backward_accumulates_into_its_outputs draws it) plus the gradient that a launch into
    zeros gives, to 2e-5 of that gradient's largest entry; rows 1.. of g_w2 / g_b2 keep the pre-fill exactly."""
    dev = gpu_device
    c = CASE['base']
    t = reference('base')[0]
    texels = texels_of(t, dev)
    d = {k: t[k].to(dev) for k in ('x', 'w1', 'b1', 'w2', 'b2', 'u_d', 'u_g')}
    zero = raw_bwd('base', texels, True)
    g = torch.Generator().manual_seed(77)
    shapes = {'g_texels': texels.shape, 'g_w1': (64, 32), 'g_b1': (64,), 'g_w2': (c.n_out, 64), 'g_b2': (c.n_out,)}
    pre = {k: torch.randn(*s, generator=g) for k, s in shapes.items()}
    out = {k: v.to(dev) for k, v in pre.items()}
    args = dict(n_scenes=c.B, points_per_scene=c.P, points=d['x'], texels=texels, plane_res=c.res,
                texel_layout=ops.texel_layout_of(texels), scene_range=range_of(c), w1=d['w1'], b1=d['b1'], w2=d['w2'],
                b2=d['b2'], g_sdf=d['u_d'], g_gradient=d['u_g'], **out)
    n_ws = _lib.struct_query('nfi_sdf_gradient_bwd_ordered_workspace_bytes', 'nfi_sdf_gradient_args', **args)
    ws = torch.full((n_ws,), 0xFF, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.call_struct('nfi_sdf_gradient_bwd_ordered', 'nfi_sdf_gradient_args', torch.cuda.current_stream(dev).cuda_stream,
                         ws, n_ws, **args)
    for k in shapes:
        assert float(zero[k].abs().max()) > 0.01, k          # so that the pre-fill's fp32 rounding stays far below the bound
        grad_close(out[k].double().cpu() - pre[k].double(), zero[k], 2e-5, 'ordered: accumulated %s - pre-fill vs launch into zeros' % k)
    assert torch.equal(out['g_w2'][1:].cpu(), pre['g_w2'][1:]) and torch.equal(out['g_b2'][1:].cpu(), pre['g_b2'][1:])


# ------------------------------------------------------------------------------------------------
# the branch: generator.regulariser_outputs of a model attached with deterministic_backward=True
# ------------------------------------------------------------------------------------------------
TERMS = ['sdf_eikonal_loss', 'sdf_distance_loss', 'total_variation_loss', 'entropy_loss']
WEIGHTS = [1.0, 0.7, 3.0, 0.01]


def branch_model(dev, deterministic, use_viewdir=False):
    torch.manual_seed(3)
    model = StandInGenerator(0.55, attention_values=10, use_sdf=True, plane_res=32, use_viewdir=use_viewdir).to(dev).train()
    nfi_gen.attach(model, **({'deterministic_backward': True} if deterministic else {}))
    z = torch.randn(2, 512, generator=torch.Generator().manual_seed(5)).to(dev)
    with torch.no_grad():
        planes = model.planes_and_values(z)[0].clone()
    assert tuple(planes.shape) == (2, 3, 32, 32, 32)
    return model, planes.requires_grad_()


def branch_gradients(model, planes):
    """The four terms and the gradients of their weighted sum w.r.t. planes, the decoder's four tensors and beta."""
    dec = model.decoder.net
    params = [planes, dec[0].weight, dec[0].bias, dec[2].weight, dec[2].bias, model.beta]
    out = nfi_gen.regulariser_outputs(model, planes, TERMS)
    assert set(out) == set(TERMS)
    return out, torch.autograd.grad(sum(w * out[n].sum() for w, n in zip(WEIGHTS, TERMS)), params)


class EntryCounter:
    """Counts _lib.call_struct's calls by entry name, and keeps the field backward's scatter_mode of each call."""

    def __init__(self, monkeypatch):
        self.calls, self.modes = {}, []
        real = _lib.call_struct

        def counted(fname, *a, **k):
            self.calls[fname] = self.calls.get(fname, 0) + 1
            if fname == 'nfi_field_query_bwd':
                self.modes.append(k.get('scatter_mode'))
            return real(fname, *a, **k)
        monkeypatch.setattr(_lib, 'call_struct', counted)


@pytest.mark.parametrize('use_viewdir', [False, True], ids=['plain', 'use_viewdir'])
def test_branch_repeats_bit_for_bit(gpu_device, monkeypatch, use_viewdir):
    """Six calls under the same seed (the branch draws its points and the total-variation perturbation itself): the
    gradients to planes, w1, b1, w2, b2 and beta are bit-identical.  Both HIP backward nodes run ordered: the
    distance-plus-gradient node through the new entry, the total-variation sampler through scatter_mode 2 (a use_viewdir
    model queries its plain distance head there)."""
    model, planes = branch_model(gpu_device, True, use_viewdir)
    count = EntryCounter(monkeypatch)
    want = None
    for call in range(6):
        torch.manual_seed(11)
        _, grads = branch_gradients(model, planes)
        assert all(float(g.abs().max()) > 0 for g in grads)
        hashes = [sha(g) for g in grads]
        want = want or hashes
        assert hashes == want, (call, [n for n, a, b in zip(['planes', 'w1', 'b1', 'w2', 'b2', 'beta'], hashes, want) if a != b])
    assert count.calls.get('nfi_sdf_gradient_bwd_ordered') == 6 and 'nfi_sdf_gradient_bwd' not in count.calls, count.calls
    assert len(count.modes) == 6 and all(m == 2 for m in count.modes), count.modes


def test_branch_against_the_float64_oracle(gpu_device):
    """test_host_api_gpu.test_regulariser_outputs with the planes as a leaf (no producer rows, a planes row) and the model
    attached with deterministic_backward=True: losses within 2e-4, gradients within 2e-3 x scale + 1e-9 of float64
    autograd of the oracle under the same two random draws."""
    model, planes = branch_model(gpu_device, True)
    draws = {}
    real_rand, real_randn_like = torch.rand, torch.randn_like

    def rand(*a, **k):
        # keeps every point off the texel boundaries, where d sdf/dx jumps (see test_regulariser_outputs)
        draws['jitter'] = real_rand(*a, **k).clamp_(1e-3, 1 - 1e-3)
        return draws['jitter']

    def randn_like(t, **k):
        draws['perturb'] = real_randn_like(t, **k)
        return draws['perturb']
    torch.rand, torch.randn_like = rand, randn_like
    try:
        out, got = branch_gradients(model, planes)
    finally:
        torch.rand, torch.randn_like = real_rand, real_randn_like
    assert tuple(draws['jitter'].shape) == (2, 31, 31, 31, 3)
    m64 = copy.deepcopy(model).cpu().double()
    d64 = m64.decoder.net
    p64 = [planes.detach().cpu().double().requires_grad_(), d64[0].weight, d64[0].bias, d64[2].weight, d64[2].bias, m64.beta]
    bins = orc.stratified_volume(2, 32, 0.55, draws['jitter'].cpu().double())
    ref = orc.regularisers(*p64[:5], bins, 0.55, True, m64.beta, draws['perturb'].cpu().double())
    for n in TERMS:
        e, tol = float((out[n].detach().cpu().double() - ref[n].detach()).abs().max()), 2e-4 * float(ref[n].detach().abs().max()) + 1e-6
        print('%-24s max %.3e (bound %.1e)' % (n, e, tol))
        assert e <= tol, (n, e, tol)
    ref_g = torch.autograd.grad(sum(w * ref[n].sum() for w, n in zip(WEIGHTS, TERMS)), p64)
    for name, a, b in zip(['planes', 'w1', 'b1', 'w2', 'b2', 'beta'], got, ref_g):
        scale, e = b.abs().max().item(), (a.cpu().double() - b).abs().max().item()
        print('grad %-19s max %.3e (bound %.1e)' % (name, e, 2e-3 * scale + 1e-9))
        assert e <= 2e-3 * scale + 1e-9, (name, e, scale)


def test_default_attach_keeps_the_atomic_entry(gpu_device, monkeypatch):
    """attach(model) without the option: the branch calls nfi_sdf_gradient_bwd and never the ordered entry."""
    model, planes = branch_model(gpu_device, False)
    count = EntryCounter(monkeypatch)
    torch.manual_seed(11)
    branch_gradients(model, planes)
    assert count.calls.get('nfi_sdf_gradient_bwd') == 1 and 'nfi_sdf_gradient_bwd_ordered' not in count.calls, count.calls
