"""CPU-side checks of the ordered hand-off and augmentation backwards: the three entries are declared, bound and exported
with the prototypes their header comments promise, the hand-off's workspace size behaves, the call refuses a missing or
short workspace before any launch, and every host switch exists, is off by default and reaches the block's flag."""
import ctypes
import inspect
import re
import types

import pytest
import torch

from nerf_from_image_amd import _lib

WARP = 'nfi_affine_warp_bwd_ordered'
SIZE, ENTRY = 'nfi_torgb_texels_bwd_ordered_workspace_bytes', 'nfi_torgb_texels_bwd_ordered'
STRUCT = 'nfi_torgb_args'


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    return _lib.load()


def size(**kw):
    return _lib.struct_query(SIZE, STRUCT, **kw)


def prototypes():
    src = _lib._strip_comments(open(_lib.HEADER).read())
    return {m.group(2): (m.group(1), [p.strip() for p in m.group(3).split(',')])
            for m in re.finditer(r'(\w+)\s+(nfi_\w+)\s*\(([^)]*)\)\s*;', src)}


def test_the_three_entries_are_declared_bound_and_exported(lib):
    proto = prototypes()
    assert proto[WARP] == proto['nfi_affine_warp_bwd'] == ('int', ['const nfi_warp_args* a', 'nfi_stream_t stream'])
    assert proto[SIZE] == ('size_t', ['const nfi_torgb_args* a'])
    assert proto[ENTRY] == ('int', ['const nfi_torgb_args* a', 'void* workspace', 'size_t workspace_bytes', 'nfi_stream_t stream'])
    assert _lib.FUNCTIONS[WARP] == _lib.FUNCTIONS['nfi_affine_warp_bwd'] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
    assert _lib.FUNCTIONS[SIZE] == (ctypes.c_size_t, [ctypes.c_void_p])
    assert _lib.FUNCTIONS[ENTRY] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p])
    for name in (WARP, SIZE, ENTRY):
        fn = getattr(lib, name)                   # AttributeError: not exported by the built library
        assert fn.restype is _lib.FUNCTIONS[name][0] and list(fn.argtypes) == _lib.FUNCTIONS[name][1]


def test_workspace_bytes(lib):
    """Positive and non-decreasing in B, R and Cin, and at least what the header comment states: 4 Cin floats per scene and
    data block of 1 024 pixels, 96 x 64 + 96 floats per block of the weight grid min(ceil(B R^2 / 64), 256) x ceil(Cin / 64)."""
    def floor_of(B, Cin, R):
        P = R * R
        blocks = min(-(-B * P // 64), 256)
        return 4 * (B * -(-P // 1024) * 4 * Cin + blocks * (-(-Cin // 64) * 96 * 64 + 96))
    Bs, Cins, Rs = (1, 2, 4, 16), (16, 144, 256), (8, 24, 40, 96, 256)
    n = {(B, Cin, R): size(n_scenes=B, in_channels=Cin, resolution=R) for B in Bs for Cin in Cins for R in Rs}
    for (B, Cin, R), v in n.items():
        assert v > 0 and v >= floor_of(B, Cin, R), (B, Cin, R, v)
    for B in Bs:
        for Cin in Cins:
            assert [n[B, Cin, R] for R in Rs] == sorted(n[B, Cin, R] for R in Rs), ('R', B, Cin)
        for R in Rs:
            assert [n[B, Cin, R] for Cin in Cins] == sorted(n[B, Cin, R] for Cin in Cins), ('Cin', B, R)
    for Cin in Cins:
        for R in Rs:
            assert [n[B, Cin, R] for B in Bs] == sorted(n[B, Cin, R] for B in Bs), ('B', Cin, R)
    assert n[4, 256, 256] > n[1, 256, 256] > n[1, 16, 256] > n[1, 16, 8]
    # a shape the call refuses has no size
    assert size(n_scenes=2, in_channels=24, resolution=40) == 0
    assert size(n_scenes=2, in_channels=32, resolution=12) == 0
    assert size(n_scenes=0, in_channels=32, resolution=40) == 0


def test_refusals_come_with_a_message_and_before_any_launch(lib):
    base = dict(n_scenes=2, in_channels=144, resolution=40, x=16, styles=16, weight=16, previous_image=16, g_texels=16, g_x=16,
                g_styles=16, g_weight=16, g_bias=16, g_previous_image=16)
    need = size(**base)
    assert need > 0

    def call(workspace, n_bytes, **kw):
        a = _lib.make_args(STRUCT, **dict(base, **kw))
        rc = lib.nfi_torgb_texels_bwd_ordered(ctypes.byref(a), workspace, n_bytes, None)
        return rc, lib.nfi_last_error()

    for workspace, n_bytes in ((None, need), (ctypes.c_void_p(256), need - 1), (ctypes.c_void_p(256), 0)):
        rc, msg = call(workspace, n_bytes)
        assert rc != 0 and b'workspace' in msg, (rc, msg)
    rc, msg = call(ctypes.c_void_p(256), need, in_channels=24)
    assert rc != 0 and b'in_channels' in msg, (rc, msg)
    rc, msg = call(ctypes.c_void_p(256), need, resolution=12)
    assert rc != 0 and b'resolution' in msg, (rc, msg)
    rc, msg = call(ctypes.c_void_p(256), need, g_styles=None)
    assert rc != 0 and b'g_styles' in msg, (rc, msg)
    with pytest.raises(RuntimeError, match='workspace'):
        _lib.call_struct(ENTRY, STRUCT, 0, None, need, **base)
    # the warp's ordered entry refuses what nfi_affine_warp_bwd refuses
    a = _lib.make_args('nfi_warp_args', n_images=2, channels=3, height=8, width=8, rot=16, translation=16)
    assert lib.nfi_affine_warp_bwd_ordered(ctypes.byref(a), None) != 0 and b'null gradient pointer' in lib.nfi_last_error()


def test_every_switch_exists_and_is_off_by_default():
    from nerf_from_image_amd import augment, handoff, ops
    default = lambda fn, name: inspect.signature(fn).parameters[name].default
    assert default(ops.affine_warp_bwd, 'ordered') is False
    assert default(ops.torgb_texels_bwd, 'ordered') is False
    assert default(augment.warp_images, 'deterministic_backward') is False
    assert default(augment.configure, 'deterministic_backward') is False
    assert default(handoff.torgb_upsample_add, 'deterministic_backward') is False
    assert default(handoff.fuse_last_block, 'deterministic_backward') is False
    before = augment.args, augment.dataset_config, augment.deterministic_backward
    try:
        augment.configure(types.SimpleNamespace(supervise_alpha=False), {'white_background': False}, deterministic_backward=True)
        assert augment.deterministic_backward is True
        augment.configure(types.SimpleNamespace(supervise_alpha=False), {'white_background': False})
        assert augment.deterministic_backward is False
    finally:
        augment.args, augment.dataset_config, augment.deterministic_backward = before


def test_attach_states_the_blocks_flag(monkeypatch):
    """attach(fused_handoff=True, deterministic_backward=True) sets the last block's flag, the block's forward hands it to
    torgb_upsample_add, and a following attach(model) clears it while the block stays fused."""
    import nerf_from_image_amd.generator as nfi_gen
    from nerf_from_image_amd import handoff
    from stand_in import StandInGenerator, StyleLikeSynthesis
    model = StandInGenerator(0.55, attention_values=10, use_sdf=True, plane_res=16)
    model.synthesis_network = StyleLikeSynthesis(16, channels=16)
    blk = model.synthesis_network.b16
    seen = []

    def tail(x, styles, weight, bias, previous_image, deterministic_backward=False):
        seen.append(deterministic_backward)
        return previous_image.new_zeros(x.shape[0], 96, x.shape[2], x.shape[3])
    monkeypatch.setattr(handoff, 'torgb_upsample_add', tail)
    ws = torch.zeros(1, 4, 512)

    nfi_gen.attach(model, fused_handoff=True)
    assert blk.nfi_deterministic_backward is False and model.nfi_deterministic_backward is False
    nfi_gen.attach(model, fused_handoff=True, deterministic_backward=True)
    assert blk.nfi_deterministic_backward is True and model.nfi_deterministic_backward is True
    model.synthesis_network(ws)
    nfi_gen.attach(model)
    assert blk.nfi_deterministic_backward is False and hasattr(blk, '_nfi_original_forward')
    model.synthesis_network(ws)
    assert seen == [True, False]
    assert handoff.fuse_last_block(model.synthesis_network, deterministic_backward=True) is blk and blk.nfi_deterministic_backward is True
    handoff.unfuse_last_block(model.synthesis_network)
    nfi_gen.attach(model, deterministic_backward=True)               # never fused again: nothing to set
    assert not hasattr(blk, '_nfi_original_forward')
