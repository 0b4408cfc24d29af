"""Several views per scene (nfi_render_args.views_per_scene), the part that needs no GPU: the field's place in the struct,
the two argument rules - refused by the kernel-name query and by nfi_render_fwd before anything is launched or
dereferenced - and the render option.  Every query below passes placeholder pointers."""
import ctypes
import types

import pytest

from nerf_from_image_amd import _lib

PTR = 16


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    return _lib.load()


def legal_call(**over):
    """A plain 6-image 64 + 64 call as ops.render_fwd fills it."""
    f = dict(n_scenes=6, height=8, width=8, n_samples=64, fine_sampling=1, white_background=1, scene_range=0.55,
             cam2world=PTR, focal=PTR, texels=PTR, plane_res=32, texel_dtype=0, decoder_image=PTR, n_attention=10,
             attention_values=PTR, use_sdf=1, beta=PTR, alpha=PTR, noise_coarse=PTR, noise_fine=PTR, noise_fine_row_stride=64,
             rgb=PTR, depth=PTR, mask=PTR, workspace=PTR, workspace_bytes=1 << 30, skip_missed_rays=1)
    f.update(over)
    return _lib.make_args('nfi_render_args', **f)


def test_the_field_sits_between_the_pinned_ends_of_the_struct():
    f = [n for n, _ in _lib.STRUCT_FIELDS['nfi_render_args']]
    assert 'views_per_scene' in f
    assert f[:4] == ['n_scenes', 'height', 'width', 'n_samples']
    assert f[-13:] == ['profile_cycles', 'ray_features', 'termination_eps', 'texel_layout', 'clock_probe', 'row_offset',
                       'full_height', 'stash_t', 'stash_sigma', 'stash_rgb', 'rays_ready', 'coords', 'normals']
    assert dict(_lib.STRUCT_FIELDS['nfi_render_args'])['views_per_scene'] is ctypes.c_int
    legal_call(views_per_scene=3)             # make_args knows the field


def test_the_version_moved_with_the_struct(lib):
    assert lib.nfi_version() >= 101


def test_the_kernel_does_not_depend_on_the_number_of_views(lib):
    names = [lib.nfi_render_kernel_name(ctypes.byref(legal_call(views_per_scene=v))) for v in (0, 1, 3)]
    assert names[0] is not None and names[0].decode().startswith('render_fwd_kernel<'), lib.nfi_last_error()
    assert names[0] == names[1] == names[2], names


@pytest.mark.parametrize('views', [4, -1])
def test_bad_view_counts_are_refused_before_any_launch(lib, views):
    """6 images are not a whole number of 4-view scenes; a negative count means nothing."""
    a = legal_call(views_per_scene=views)
    assert lib.nfi_render_kernel_name(ctypes.byref(a)) is None
    assert b'views_per_scene' in lib.nfi_last_error()
    # as test_abi.py::test_bad_arguments_are_rejected_before_any_launch: nothing behind the placeholders is touched
    b = _lib.make_args('nfi_render_args', n_scenes=6, height=4, width=4, n_samples=16, fine_sampling=0, cam2world=PTR, rgb=PTR,
                       depth=PTR, mask=PTR, workspace=PTR, views_per_scene=views)
    assert lib.nfi_render_fwd(ctypes.byref(b), None) == -1
    assert b'views_per_scene' in lib.nfi_last_error()


def test_the_render_option():
    import nerf_from_image_amd.render as nfi_render
    cfg = types.SimpleNamespace(use_viewdir=False, use_sdf=True, attention_values=10, fine_sampling=True)
    dcfg = {'scene_range': 0.55, 'white_background': True}
    assert nfi_render.make_render(cfg, dcfg, views_per_scene=3).options.views_per_scene == 3
    assert nfi_render.make_render(cfg, dcfg).options.views_per_scene == 1
    with pytest.raises(TypeError):
        nfi_render.make_render(cfg, dcfg, views_per_sceen=3)
