"""CPU-side checks of the entries behind the renderer's neighbours in the inversion loop - nfi_pose_pnp, nfi_image_metrics,
nfi_affine_warp_fwd / _bwd and nfi_torgb_texels_fwd / _bwd: every malformed argument is refused before any launch (the
pointers below are fake, so a call that got past its checks would not come back with a message), with a non-zero return
code and the words in nfi_last_error() that name what was wrong."""
import ctypes

import pytest

from nerf_from_image_amd import _lib

FAKE = 256            # a non-null, 8-byte aligned address that is never dereferenced


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    return _lib.load()


def refused(lib, entry, struct, *words, **fields):
    """The call returns non-zero and nfi_last_error() holds every one of `words`."""
    a = _lib.make_args(struct, **fields)
    rc = getattr(lib, entry)(ctypes.byref(a), None)
    msg = lib.nfi_last_error()
    assert rc != 0, (entry, fields)
    for w in words:
        assert w.encode() in msg, (entry, w, msg)
    return msg


# ------------------------------------------------------------------------------------------------
# nfi_pose_pnp
# ------------------------------------------------------------------------------------------------
PNP_B, PNP_NF = 3, 5
PNP_POINTERS = ('coords', 'mask', 'focal_proposals', 'world2cam', 'focal', 'error', 'workspace')


def pnp_base(lib, **kw):
    d = dict(n_images=PNP_B, height=20, width=36, mask_threshold=0.5, n_focal=PNP_NF, refine_iterations=30,
             workspace_bytes=lib.nfi_pnp_workspace_bytes(PNP_B, PNP_NF), **{p: FAKE for p in PNP_POINTERS})
    d.update(kw)
    return d


def test_pnp_workspace_bytes(lib):
    """16 doubles per image and focal proposal (R, t, rmse, valid, n, focal)."""
    for B, nf in ((1, 1), (3, 5), (4, 64), (70, 1), (1000, 11)):
        assert lib.nfi_pnp_workspace_bytes(B, nf) == B * nf * 16 * 8, (B, nf)


@pytest.mark.parametrize('name', PNP_POINTERS)
def test_pnp_refuses_a_null_pointer(lib, name):
    refused(lib, 'nfi_pose_pnp', 'nfi_pnp_args', 'pose_pnp', 'null pointer', **pnp_base(lib, **{name: None}))


@pytest.mark.parametrize('name', ['n_images', 'height', 'width', 'n_focal'])
def test_pnp_refuses_an_empty_shape(lib, name):
    refused(lib, 'nfi_pose_pnp', 'nfi_pnp_args', 'pose_pnp', 'focal proposals', **pnp_base(lib, **{name: 0}))


def test_pnp_focal_proposal_limit(lib):
    """65 proposals are refused as such; 64 pass that check, and the next one (the workspace, sized for 5) refuses."""
    refused(lib, 'nfi_pose_pnp', 'nfi_pnp_args', '1..64 focal proposals', **pnp_base(lib, n_focal=65, workspace_bytes=1 << 30))
    msg = refused(lib, 'nfi_pose_pnp', 'nfi_pnp_args', 'workspace too small', **pnp_base(lib, n_focal=64))
    assert b'focal proposals' not in msg


@pytest.mark.parametrize('iterations', [-1, 201])
def test_pnp_refuses_refine_iterations_outside_0_200(lib, iterations):
    refused(lib, 'nfi_pose_pnp', 'nfi_pnp_args', 'refine_iterations', '[0,200]', **pnp_base(lib, refine_iterations=iterations))


def test_pnp_refuses_a_short_or_misaligned_workspace(lib):
    need = lib.nfi_pnp_workspace_bytes(PNP_B, PNP_NF)
    refused(lib, 'nfi_pose_pnp', 'nfi_pnp_args', 'workspace too small', **pnp_base(lib, workspace_bytes=need - 1))
    refused(lib, 'nfi_pose_pnp', 'nfi_pnp_args', 'workspace too small', **pnp_base(lib, workspace_bytes=0))
    for address in (FAKE + 4, FAKE + 1, FAKE + 7):
        refused(lib, 'nfi_pose_pnp', 'nfi_pnp_args', 'workspace', '8-byte aligned', **pnp_base(lib, workspace=address))
    with pytest.raises(RuntimeError, match='8-byte aligned'):
        _lib.call_struct('nfi_pose_pnp', 'nfi_pnp_args', 0, **pnp_base(lib, workspace=FAKE + 4))


# ------------------------------------------------------------------------------------------------
# nfi_image_metrics
# ------------------------------------------------------------------------------------------------
METRICS_PSNR = dict(pred=FAKE, target=FAKE, elements_per_image=969, psnr=FAKE)
METRICS_IOU = dict(mask_pred=FAKE, mask_real=FAKE, elements_per_mask=323, iou=FAKE)


def test_metrics_refuse_no_images_and_nothing_requested(lib):
    everything = dict(n_images=2, out_of_range=FAKE, **METRICS_PSNR, **METRICS_IOU)
    for n in (0, -1):
        refused(lib, 'nfi_image_metrics', 'nfi_metrics_args', 'image_metrics', 'bad shape', **dict(everything, n_images=n))
    refused(lib, 'nfi_image_metrics', 'nfi_metrics_args', 'nothing requested', **dict(everything, psnr=None, iou=None))


@pytest.mark.parametrize('other', [False, True], ids=['alone', 'with_the_other_metric'])
@pytest.mark.parametrize('missing', ['pred', 'target', 'elements_per_image'])
def test_metrics_refuse_psnr_without_its_inputs(lib, missing, other):
    kw = dict(n_images=2, out_of_range=FAKE, **METRICS_PSNR, **(METRICS_IOU if other else {}))
    kw[missing] = 0 if missing.startswith('elements') else None
    refused(lib, 'nfi_image_metrics', 'nfi_metrics_args', 'psnr inputs missing', **kw)


@pytest.mark.parametrize('other', [False, True], ids=['alone', 'with_the_other_metric'])
@pytest.mark.parametrize('missing', ['mask_pred', 'mask_real', 'elements_per_mask'])
def test_metrics_refuse_iou_without_its_inputs(lib, missing, other):
    kw = dict(n_images=2, out_of_range=FAKE, **METRICS_IOU, **(METRICS_PSNR if other else {}))
    kw[missing] = 0 if missing.startswith('elements') else None
    refused(lib, 'nfi_image_metrics', 'nfi_metrics_args', 'iou inputs missing', **kw)


# ------------------------------------------------------------------------------------------------
# nfi_affine_warp_fwd / nfi_affine_warp_bwd
# ------------------------------------------------------------------------------------------------
WARP_BASE = dict(n_images=7, channels=9, height=33, width=65, image=FAKE, warped=FAKE, g_warped=FAKE, g_image=FAKE, rot=FAKE,
                 scale=FAKE, translation=FAKE, white_background=1)
WARP_ENTRIES = ['nfi_affine_warp_fwd', 'nfi_affine_warp_bwd']


@pytest.mark.parametrize('entry', WARP_ENTRIES)
def test_warp_refuses_a_missing_transform(lib, entry):
    for name in ('rot', 'translation'):
        refused(lib, entry, 'nfi_warp_args', 'affine_warp', 'null pointer', **dict(WARP_BASE, **{name: None}))


@pytest.mark.parametrize('entry', WARP_ENTRIES)
@pytest.mark.parametrize('name', ['n_images', 'channels', 'height', 'width'])
def test_warp_refuses_an_empty_shape(lib, entry, name):
    refused(lib, entry, 'nfi_warp_args', 'affine_warp', 'bad shape', **dict(WARP_BASE, **{name: 0}))


@pytest.mark.parametrize('entry', WARP_ENTRIES)
def test_warp_refuses_2_to_the_30_pixels(lib, entry):
    """The kernels index a plane with an int: height * width stays below 2^30."""
    for H, W in ((32768, 32768), (1, 1 << 30), (1 << 30, 1), (65536, 65536)):
        refused(lib, entry, 'nfi_warp_args', 'image too large', **dict(WARP_BASE, height=H, width=W))


def test_warp_refuses_a_missing_image_or_gradient(lib):
    for name in ('image', 'warped'):
        refused(lib, 'nfi_affine_warp_fwd', 'nfi_warp_args', 'affine_warp_fwd', 'null image pointer', **dict(WARP_BASE, **{name: None}))
    for name in ('g_warped', 'g_image'):
        refused(lib, 'nfi_affine_warp_bwd', 'nfi_warp_args', 'affine_warp_bwd', 'null gradient pointer', **dict(WARP_BASE, **{name: None}))


# ------------------------------------------------------------------------------------------------
# nfi_torgb_texels_fwd / nfi_torgb_texels_bwd
# ------------------------------------------------------------------------------------------------
TORGB_BASE = dict(n_scenes=2, in_channels=144, resolution=40, x=FAKE, styles=FAKE, weight=FAKE, bias=FAKE, previous_image=FAKE,
                  texels=FAKE, g_texels=FAKE, g_x=FAKE, g_styles=FAKE, g_weight=FAKE, g_bias=FAKE, g_previous_image=FAKE)
TORGB_ENTRIES = ['nfi_torgb_texels_fwd', 'nfi_torgb_texels_bwd']


@pytest.mark.parametrize('entry', TORGB_ENTRIES)
@pytest.mark.parametrize('channels', [8, 24, 272])
def test_torgb_refuses_in_channels(lib, entry, channels):
    refused(lib, entry, 'nfi_torgb_args', 'torgb_texels', 'in_channels', 'multiple of 16', **dict(TORGB_BASE, in_channels=channels))


@pytest.mark.parametrize('entry', TORGB_ENTRIES)
@pytest.mark.parametrize('resolution', [4, 12, 1032])
def test_torgb_refuses_resolution(lib, entry, resolution):
    refused(lib, entry, 'nfi_torgb_args', 'torgb_texels', 'resolution', 'multiple of 8', **dict(TORGB_BASE, resolution=resolution))


def test_torgb_forward_refuses_a_missing_bias_or_output(lib):
    for name in ('bias', 'texels'):
        refused(lib, 'nfi_torgb_texels_fwd', 'nfi_torgb_args', 'torgb_texels_fwd', 'null pointer', **dict(TORGB_BASE, **{name: None}))


def test_torgb_backward_refuses_a_weight_gradient_without_the_bias_gradient(lib):
    """Both or neither (include/nfi_hip.h) - and refused like everything else: before the first memset and launch."""
    refused(lib, 'nfi_torgb_texels_bwd', 'nfi_torgb_args', 'torgb_texels_bwd', 'g_bias', **dict(TORGB_BASE, g_bias=None))
    refused(lib, 'nfi_torgb_texels_bwd', 'nfi_torgb_args', 'torgb_texels_bwd', 'g_bias', **dict(TORGB_BASE, g_bias=None, previous_image=None,
                                                                                               g_previous_image=None))
