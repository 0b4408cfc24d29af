"""CPU-side checks of the regulariser's ordered backward at the C ABI: both entries are exported with the header's
prototypes, the workspace size behaves, and the call refuses what its header comment says it refuses - before any launch."""
import ctypes
import re

import pytest

from nerf_from_image_amd import _lib

STRUCT = 'nfi_sdf_gradient_args'
SIZE, ENTRY = 'nfi_sdf_gradient_bwd_ordered_workspace_bytes', 'nfi_sdf_gradient_bwd_ordered'


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    return _lib.load()


def size(**kw):
    return _lib.struct_query(SIZE, STRUCT, **kw)


def test_both_entries_are_exported_with_the_header_prototypes(lib):
    src = _lib._strip_comments(open(_lib.HEADER).read())
    proto = {m.group(2): (m.group(1), [p.strip() for p in m.group(3).split(',')])
             for m in re.finditer(r'(\w+)\s+(nfi_sdf_gradient_bwd_ordered\w*)\s*\(([^)]*)\)\s*;', src)}
    assert proto == {SIZE: ('size_t', ['const nfi_sdf_gradient_args* a']),
                     ENTRY: ('int', ['const nfi_sdf_gradient_args* a', 'void* workspace', 'size_t workspace_bytes', 'nfi_stream_t stream'])}
    assert _lib.FUNCTIONS[SIZE] == (ctypes.c_size_t, [ctypes.c_void_p])
    assert _lib.FUNCTIONS[ENTRY] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p])
    for name in (SIZE, ENTRY):
        fn = getattr(lib, name)
        assert fn.restype is _lib.FUNCTIONS[name][0] and list(fn.argtypes) == _lib.FUNCTIONS[name][1]
    # the argument struct keeps its layout: the ordered entry reads the one nfi_sdf_gradient_bwd reads
    assert [n for n, _ in _lib.STRUCT_FIELDS[STRUCT]] == [
        'n_scenes', 'points_per_scene', 'points', 'texels', 'plane_res', 'scene_range', 'w1', 'b1', 'w2', 'b2', 'sdf', 'gradient',
        'g_sdf', 'g_gradient', 'g_texels', 'g_w1', 'g_b1', 'g_w2', 'g_b2', 'texel_layout']


def test_workspace_bytes(lib):
    """Non-zero, non-decreasing in points_per_scene and n_scenes, and at least what the header comment states: per point
    two rows of 128 B, a flag byte and two 8-byte keys for each of the three planes; per wave of the grid a slot of 2 192
    floats (the grid has at least one block of four waves per scene)."""
    per_point, per_wave = 2 * 128 + 1 + 2 * 3 * 8, 2192 * 4
    last = 0
    for P in (1, 63, 64, 65, 1000, 5003, 29791, 29792, 1 << 20, 1 << 25):
        n = size(n_scenes=4, points_per_scene=P, plane_res=256)
        assert n > 0 and n >= last and n >= 4 * P * per_point + 4 * 4 * per_wave, (P, n)
        last = n
    last = 0
    for B in (1, 2, 3, 4, 16, 17, 64, 300):
        n = size(n_scenes=B, points_per_scene=29791, plane_res=256)
        assert n > 0 and n >= last and n >= B * 29791 * per_point + B * 4 * per_wave, (B, n)
        last = n
    # the full grid of 4 x 31^3 points: 64 blocks per scene
    assert size(n_scenes=4, points_per_scene=29791, plane_res=256) >= 4 * 29791 * per_point + 4 * 64 * 4 * per_wave
    # a shape the call refuses has no size
    assert size(n_scenes=1, points_per_scene=(1 << 25) + 1, plane_res=256) == 0


def test_refusals_come_with_a_message_and_before_any_launch(lib):
    base = dict(n_scenes=2, points_per_scene=200, plane_res=24, scene_range=0.55, points=16, texels=16, w1=16, b1=16, w2=16, b2=16,
                g_sdf=16, g_gradient=16, g_texels=16, g_w1=16, g_b1=16, g_w2=16, g_b2=16)
    need = size(**base)

    def call(workspace, n_bytes, **kw):
        a = _lib.make_args(STRUCT, **dict(base, **kw))
        rc = lib.nfi_sdf_gradient_bwd_ordered(ctypes.byref(a), workspace, n_bytes, None)
        return rc, lib.nfi_last_error()

    rc, msg = call(None, need)
    assert rc == -1 and b'workspace missing' in msg, (rc, msg)
    rc, msg = call(ctypes.c_void_p(256), need - 1)
    assert rc == -1 and b'workspace too small' in msg, (rc, msg)
    rc, msg = call(ctypes.c_void_p(256), 0)
    assert rc == -1 and b'workspace too small' in msg, (rc, msg)
    rc, msg = call(ctypes.c_void_p(256), need, g_sdf=None, g_gradient=None)
    assert rc == -1 and b'no upstream gradient' in msg, (rc, msg)
    rc, msg = call(ctypes.c_void_p(256), 1 << 40, points_per_scene=(1 << 25) + 1)
    assert rc == -1 and b'2^25' in msg, (rc, msg)
    with pytest.raises(RuntimeError, match='workspace missing'):
        _lib.call_struct(ENTRY, STRUCT, 0, None, need, **base)
