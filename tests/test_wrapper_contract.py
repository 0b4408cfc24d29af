"""The wrapper contract without a GPU: the table of tests/contract_util.py is complete and consistent, host tensors never
reach a launching entry, and the view helpers do what the GPU cases rely on."""
import pytest
import torch

import contract_util as cu
from nerf_from_image_amd import _lib, ops


def test_every_wrapper_that_reaches_the_library_has_a_row_or_a_reason():
    reach = cu.wrappers_that_reach_the_library()
    assert {'field_query', 'render_fwd', 'sdf_gradient_bwd', 'torgb_texels_bwd', 'texel_grad_to_planes', 'raygen_bwd'} <= reach
    with_row = {r.fn for r in cu.ROWS}
    missing = sorted(reach - with_row - set(cu.EXEMPT))
    assert not missing, 'public wrappers of ops.py without a row in tests/contract_util.py (or a reason in EXEMPT): %s' % missing
    assert 'field_query_bwd' in with_row                            # field_backward's, the one wrapper outside ops.py
    stale = sorted(n for n in set(cu.EXEMPT) | (with_row - {'field_query_bwd'}) if not callable(getattr(ops, n, None)))
    assert not stale, 'rows / exemptions for functions ops.py does not have: %s' % stale
    both = sorted(with_row & set(cu.EXEMPT))
    assert not both, both
    assert len(set(cu.ROW_IDS)) == len(cu.ROW_IDS)


def test_a_wrapper_without_a_row_is_noticed(monkeypatch):
    """The completeness check bites: with one row's function taken out of the table it names that function."""
    left = [r for r in cu.ROWS if r.fn != 'points_bwd']
    assert len(left) < len(cu.ROWS)
    assert 'points_bwd' in cu.wrappers_that_reach_the_library() - {r.fn for r in left} - set(cu.EXEMPT)


STAND_IN = '''
from nerf_from_image_amd import _lib


def _hand_over(kw):
    _lib.call_struct('nfi_x', 'nfi_x_args', 0, **kw)


def _twice_removed(kw):
    return _hand_over(kw)


def through_a_private_helper(x):
    return _hand_over(dict(x=x))


def through_two_private_helpers(x):
    return _twice_removed(dict(x=x))


def through_a_public_wrapper(x):
    return through_a_private_helper(x)


def straight(x):
    _lib.call_struct('nfi_x', 'nfi_x_args', 0, x=x)


def checks_only(x):
    return x
'''


def test_a_wrapper_whose_only_way_to_the_library_is_a_private_helper_is_noticed(tmp_path):
    """The completeness check follows the module's private helpers: a public function that reaches _lib only through
    `_something(...)` is found, and without a row or a reason it is reported as missing.  (A stand-in module: ops.py's own
    names are not restated here.)"""
    import importlib.util
    path = tmp_path / 'contract_stand_in.py'
    path.write_text(STAND_IN)
    spec = importlib.util.spec_from_file_location('contract_stand_in', str(path))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    reach = cu.wrappers_that_reach_the_library(module)
    assert reach == {'through_a_private_helper', 'through_two_private_helpers', 'through_a_public_wrapper', 'straight'}
    missing = reach - {r.fn for r in cu.ROWS} - set(cu.EXEMPT)
    assert {'through_a_private_helper', 'through_two_private_helpers'} <= missing
    # ... and in ops.py itself every launcher that takes a checked dict is public, seen, and exempt through its wrapper
    launchers = {n for n in cu.wrappers_that_reach_the_library() if n.endswith('_launch')}
    assert launchers and launchers <= set(cu.EXEMPT)
    assert all(cu.EXEMPT[n].rsplit(' ', 1)[-1] in {r.fn for r in cu.ROWS} for n in launchers)


def test_launching_entries_are_told_from_size_queries():
    launching = cu.stream_entries()
    assert {'nfi_render_fwd', 'nfi_field_query_bwd', 'nfi_points_on_rays', 'nfi_sdf_gradient_bwd_ordered', 'nfi_raygen_bwd'} <= launching
    for name in ('nfi_decoder_image_floats', 'nfi_decoder_image_floats_viewdir', 'nfi_render_workspace_bytes',
                 'nfi_field_bwd_workspace_bytes', 'nfi_sdf_gradient_bwd_ordered_workspace_bytes', 'nfi_version', 'nfi_last_error'):
        assert name in _lib.FUNCTIONS and name not in launching, name
    assert launching <= set(_lib.FUNCTIONS)


@pytest.mark.parametrize('rid', cu.ROW_IDS)
def test_rows_are_consistent(rid):
    """Every tensor argument a row names is a tensor of its builder, as long as the row says the wrapper must insist on; the
    builder is seeded."""
    row = cu.ROWS[cu.ROW_IDS.index(rid)]
    a, again = row.build('cpu'), row.build('cpu')
    for name, count in row.counts.items():
        assert torch.is_tensor(a[name]), name
        assert cu.bit_equal(a[name], again[name]), name
        if count is not None:
            assert a[name].numel() == count(a), (name, tuple(a[name].shape), count(a))
        assert row.widest[name] in (4, 8, 16)


@pytest.mark.parametrize('rid', cu.ROW_IDS)
def test_host_tensors_are_refused_before_any_launch(rid, monkeypatch):
    row = cu.ROWS[cu.ROW_IDS.index(rid)]
    args = row.build('cpu')
    proxy = cu.install_proxy(monkeypatch)
    with pytest.raises((RuntimeError, TypeError, ValueError)):
        row.call(args)
    assert proxy.reached == []


def test_the_proxy_stops_a_launch_and_passes_size_queries(monkeypatch):
    proxy = cu.install_proxy(monkeypatch)
    plain, viewdir = proxy.nfi_decoder_image_floats(), proxy.nfi_decoder_image_floats_viewdir()
    assert _lib.load() is proxy and plain > 0 and viewdir > 0 and plain != viewdir      # (the two images tell apart by length)
    assert proxy.nfi_render_workspace_bytes(96) > 0
    with pytest.raises(cu.ReachedLibrary, match='nfi_points_on_rays'):
        proxy.nfi_points_on_rays(None, None, None, 0, 0, None, None)
    assert proxy.reached == ['nfi_points_on_rays']


SHAPES = [(7,), (5, 6), (2, 3, 4, 4, 32), (2, 4, 4, 3, 32), (1,)]


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_view_helpers(shape, dtype):
    t = torch.randn(*shape, generator=torch.Generator().manual_seed(len(shape))).to(dtype)
    several = t.numel() > 1
    s, p, o = cu.strided(t), cu.permuted(t), cu.offset(t)
    for v in (s, p, o):
        assert v.shape == t.shape and v.dtype == t.dtype and cu.bit_equal(v, t)
    assert s.is_contiguous() == (not several)
    assert p.is_contiguous() == (not several)
    if len(shape) >= 2:
        assert p.stride(0) == 1 and p.permute(*reversed(range(len(shape)))).is_contiguous()      # dense behind the permute
    assert s.data_ptr() % 16 == 0 and p.data_ptr() % 16 == 0
    assert o.is_contiguous() and o.data_ptr() % 16 == t.element_size()
    assert cu.strided(None) is None and cu.permuted(None) is None and cu.offset(None) is None


def test_other_layout_view():
    planar = torch.randn(2, 3, 4, 4, 32, generator=torch.Generator().manual_seed(0))
    inter = planar.permute(0, 2, 3, 1, 4).contiguous()
    for t, code in ((planar, ops.TEXELS_PLANAR), (inter, ops.TEXELS_INTERLEAVED)):
        v = cu.other_layout_view(t)
        assert v.shape == t.shape and cu.bit_equal(v, t) and not v.is_contiguous() and ops.texel_layout_of(v) == code
    assert cu.other_layout_view(planar).permute(0, 2, 3, 1, 4).is_contiguous()


def test_pose_util_keeps_its_strided():
    import pose_util
    assert pose_util.strided is cu.strided
