"""tools/xcd_balance.py, the CPU census of the render kernels' per-XCD hand-out, on the benchmark's own cameras."""
import importlib.util
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_tool():
    spec = importlib.util.spec_from_file_location('xcd_balance', os.path.join(ROOT, 'tools', 'xcd_balance.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bench_seed_census(capsys):
    """the benchmark's cameras (seed 1234): the recorded per-XCD marched rays in today's order, max/mean <= 1.05 paired"""
    tool = load_tool()
    cam, focal = tool.bench_cameras(1234)
    c = tool.census(cam, focal, 128, 128, 0.55)
    assert c['in_order'] == [5434, 12280, 12816, 5674, 5713, 12976, 12923, 5752]
    assert sum(c['paired']) == sum(c['in_order']) == 73568
    print('paired', c['paired'], tool.spread(c['paired']))
    assert tool.spread(c['paired']) <= 1.05
    assert tool.main([]) == 0
    out = capsys.readouterr().out
    assert '5434 12280 12816 5674 5713 12976 12923 5752' in out
    assert float(out.strip().rsplit(' ', 1)[1]) <= 1.05


def test_paired_table_rule():
    """the table is a permutation of every aligned group of 16, ties go by index, an incomplete group stays in order"""
    tool = load_tool()
    counts = torch.tensor([5] * 16 + list(range(16)) + [9, 1, 7])
    t = tool.paired_table(counts)
    assert sorted(t[:16]) == list(range(16)) and sorted(t[16:32]) == list(range(16, 32)) and t[32:] == [32, 33, 34]
    # all counts equal: rank = index; group 0 puts rank r < 8 in slot r and rank 15 - r in slot 8 + r
    assert t[:16] == [0, 1, 2, 3, 4, 5, 6, 7, 15, 14, 13, 12, 11, 10, 9, 8]
    # group 1, counts 0..15 ascending: rank r is block 31 - r, the pairs move on by one XCD
    assert t[16:32] == [31 - 7, 31, 30, 29, 28, 27, 26, 25, 16 + 7, 16, 17, 18, 19, 20, 21, 22]
