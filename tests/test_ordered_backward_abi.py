"""The ordered backward (nfi_field_bwd_args.scatter_mode 2, nfi_raygen_bwd_ordered, the render option
deterministic_backward) at the boundary: declared, exported, sized and refused without a GPU."""
import re
import types

import pytest
import torch

from nerf_from_image_amd import _lib


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    return _lib.load()


def workspace_bytes(P, mode, B=2, res=24, **kw):
    return _lib.struct_query('nfi_field_bwd_workspace_bytes', 'nfi_field_bwd_args', n_scenes=B, points_per_scene=P,
                             plane_res=res, scatter_mode=mode, **kw)


def test_header_declares_and_library_exports_the_ordered_raygen_backward(lib):
    declared = set(re.findall(r'\b(nfi_[a-z_0-9]+)\s*\(', open(_lib.HEADER).read()))
    assert 'nfi_raygen_bwd_ordered' in declared and 'nfi_raygen_bwd_ordered' in _lib.FUNCTIONS
    assert _lib.FUNCTIONS['nfi_raygen_bwd_ordered'] == _lib.FUNCTIONS['nfi_raygen_bwd']      # same signature
    assert hasattr(lib, 'nfi_raygen_bwd_ordered')


def test_workspace_query_answers_for_the_ordered_mode(lib):
    B, P = 2, 5000
    plain, binned, ordered = (workspace_bytes(P, m) for m in (0, 1, 2))
    assert ordered > plain > 0
    # at least the rows (128 B per point) and the flag bytes the binned mode's answer contains
    assert ordered >= plain + B * P * (128 + 1) and binned >= plain + B * P * (128 + 1)
    # monotone in P, also across the sizes at which the grid - and with it the number of per-wave slots - stops growing
    sizes = [1, 63, 64, 65, 1000, 4999, 5000, 5001, 8229, 65536, 70000, 1 << 20, 1 << 25]
    answers = [workspace_bytes(p, 2) for p in sizes]
    assert all(a <= b for a, b in zip(answers, answers[1:])), answers
    # nothing to order: the answer is the operand image's, as in mode 0
    assert workspace_bytes(P, 2, points_only=1) == workspace_bytes(P, 0, points_only=1)


def test_wrapper_refuses_the_ordered_mode_for_viewdir_and_points_only_without_a_device():
    """Before any tensor is looked at: CPU tensors would otherwise fail the device check with a RuntimeError."""
    from nerf_from_image_amd.field_backward import field_query_bwd
    B, P, A = 1, 8, 10
    z = torch.zeros
    args = (z(B, P, 3), z(B, 3, 4, 4, 32), z(8), z(64, 32), z(1 + A, 64), 0.55, A, z(B, A, 3), True, z(1), z(1), z(B, P), z(B, P, 3))
    with pytest.raises(NotImplementedError, match='ordered'):
        field_query_bwd(*args, scatter_mode=2, points_only=True)
    with pytest.raises(NotImplementedError, match='ordered'):
        field_query_bwd(*args, scatter_mode=2, viewdir=dict(ray_features=z(B, 1, 48), samples_per_ray=P, w3=z(A, 32)))


def test_render_option_deterministic_backward_is_known_and_off_by_default():
    import nerf_from_image_amd.render as nfi_render
    cfg = types.SimpleNamespace(use_viewdir=False, use_sdf=True, attention_values=10, fine_sampling=True)
    dcfg = {'scene_range': 0.55, 'white_background': True}
    assert nfi_render.make_render(cfg, dcfg).options.deterministic_backward is False
    assert nfi_render.make_render(cfg, dcfg, deterministic_backward=True).options.deterministic_backward is True
    with pytest.raises(TypeError, match='unknown render option'):
        nfi_render.make_render(cfg, dcfg, deterministic_backwards=True)


PTR = 16      # never dereferenced: the argument rules look at nulls and integers only


def legal_call(**kw):
    f = dict(n_scenes=2, points_per_scene=200, points=PTR, texels=PTR, plane_res=24, texel_dtype=0, decoder_image=PTR, w1=PTR,
             w2=PTR, n_attention=10, attention_values=PTR, use_sdf=1, beta=PTR, alpha=PTR, scene_range=0.55, g_sigma=PTR,
             g_rgb=PTR, g_texels=PTR, g_points=PTR, g_w1=PTR, g_b1=PTR, g_w2=PTR, g_b2=PTR, g_attention_values=PTR, g_beta=PTR,
             g_alpha=PTR, workspace=PTR, workspace_bytes=1 << 30)
    f.update(kw)
    return _lib.make_args('nfi_field_bwd_args', **f)


def test_argument_rules_of_the_ordered_mode(lib):
    import ctypes
    name = lambda a: lib.nfi_field_bwd_kernel_name(ctypes.byref(a))
    # the ordered mode picks among the same 16 kernels: no instantiation of its own
    assert name(legal_call(scatter_mode=2)) == name(legal_call(scatter_mode=0)) == b'field_query_bwd_kernel<1,1,0,0>'
    for bad in (3, -1):
        assert name(legal_call(scatter_mode=bad)) is None and b'scatter_mode' in lib.nfi_last_error()
    vd = dict(ray_features=PTR, samples_per_ray=8, w3=PTR, g_ray_features=PTR, g_w3=PTR, g_b3=PTR)
    assert name(legal_call(scatter_mode=1, **vd)) is not None
    assert name(legal_call(scatter_mode=2, **vd)) is None and b'view-direction' in lib.nfi_last_error()
    assert name(legal_call(scatter_mode=0, points_only=1)) is not None
    assert name(legal_call(scatter_mode=2, points_only=1)) is None and b'points_only' in lib.nfi_last_error()
    # the limit of 2^25 points per scene is the binned mode's
    big = (1 << 25) + 64
    assert name(legal_call(scatter_mode=0, points_per_scene=big, workspace_bytes=1 << 62)) is not None
    assert name(legal_call(scatter_mode=2, points_per_scene=big, workspace_bytes=1 << 62)) is None and b'2^25' in lib.nfi_last_error()
    # and the workspace is checked against the mode's own answer
    need = workspace_bytes(200, 2)
    assert name(legal_call(scatter_mode=2, workspace_bytes=need)) is not None
    assert name(legal_call(scatter_mode=2, workspace_bytes=need - 1)) is None and b'workspace' in lib.nfi_last_error()


def test_attach_hands_the_switch_to_the_sampler_closure():
    import inspect
    import nerf_from_image_amd.generator as nfi_gen
    from nerf_from_image_amd.field_backward import make_field_bwd
    from stand_in import StandInGenerator
    model = StandInGenerator(0.55, plane_res=8)
    assert nfi_gen._sampler_options(nfi_gen.attach(model)) == {}
    assert nfi_gen._sampler_options(nfi_gen.attach(model, deterministic_backward=True)) == {'deterministic_backward': True}
    assert nfi_gen._sampler_options(nfi_gen.attach(model)) == {}                       # off again: attach states the whole configuration
    assert inspect.signature(nfi_gen.make_sampler).parameters['deterministic_backward'].default is False
    assert inspect.signature(make_field_bwd).parameters['scatter_mode'].default is None
