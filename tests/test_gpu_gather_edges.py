"""csrc/gather.hip on table borders, empty voxels, ragged counts and long runs, on the MI355X: the `check_*` bodies of tests/test_hipcpu_gather_edges.py
(which runs them on the host build), here against libsherf_hip.so on the device -- and the cases only a device of this size reaches: a wave of the run-order
scatter that carries its running sums across a chunk boundary (per > 1: above 64 * 16 * CUs samples, 262 144 on an MI355X), and the forward kernels'
grid-stride tile loops past their caps of 16 384 workgroups.  Both use a PERIODIC input: a base of 4096 samples (every group of the synthetic scene,
checked against float64 on its own) repeated, so that the expected result follows from the base's and the comparison stays on the device.

Not covered at its cap: the LDS-staged form (debug bit 29), whose 16 384 workgroups x 4 pairs of tiles need 4.2 M samples = 1.6 GB of tokens; its
workgroups walk several pairs of tiles at every size, so its loop makes its further trips in every case of check_forward."""
import pytest
import torch

from tests import gpu_common as G
from tests import test_hipcpu_gather_edges as E

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]

PERIOD = 4096                                             # 128 whole tiles


@pytest.mark.parametrize('n', E.RAGGED)
def test_ragged_counts_forward(n):
    E.check_ragged_forward(n)


@pytest.mark.parametrize('n', E.RAGGED)
def test_ragged_counts_backward(n):
    E.check_ragged_backward(n)


def test_count_above_capacity():
    E.check_overflowing_count()


def test_long_run_forward():
    E.check_long_run_forward()


def test_long_run_backward():
    E.check_long_run_backward()


def test_second_scan_trip():
    E.check_second_scan_trip()


def test_base_period_against_float64():
    """The 4096 samples the periodic cases repeat, on their own: every forward form and the three scatters."""
    sc, dev = E.scene_on_device('base4096')
    assert sc.n == PERIOD and all(g.numel() for g in sc.groups.values())
    E.check_forward(sc, dev, 'base 4096')
    E.check_backward(sc, dev, 'base 4096')


def test_multi_chunk_walk():
    """n = 64 * (16 * CUs + 3) + 5: the smallest count at which a wave of gather_tokens_bwd_runs_kernel walks two chunks (the launch arithmetic of
    sherf_gather_tokens_bwd_binned restated below), i.e. keeps running sums, current cells and target lanes across a chunk boundary.  The sorted order
    puts each cell's samples of all repeats next to each other: the one-cell group becomes a run of 160 K samples over thousands of chunks."""
    sc, dev = E.scene_on_device('base4096')
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 64 * (16 * cus + 3) + 5
    chunks = (n + 63) // 64
    grid = min(chunks // 4 + 1, 4 * cus)
    per = -(-chunks // (4 * grid))
    assert per >= 2, (cus, n, grid, per)
    reps, tail = divmod(n, PERIOD)
    geom = torch.cat([dev.geom.repeat(reps, 1), dev.geom[:tail]]).contiguous()
    base = E.tile_tokens(sc.d_tok, PERIOD // 32).cuda()
    d_tiled = torch.cat([base.repeat(reps), E.tile_tokens(sc.d_tok[:tail], (tail + 31) // 32).cuda()]).contiguous()
    assert geom.shape[0] == n and d_tiled.numel() == ((n + 31) // 32) * 3072
    out, scratch, bins = dev.backward(n, n, d_tiled, 'runs', geom=geom)
    cells = E.assert_scratch('multi-chunk', scratch, bins, n, n, 'runs')
    assert int(torch.bincount(cells).max()) >= reps * sc.groups['run'].numel()
    E.assert_backward(sc, f'multi-chunk n={n} runs', out, PERIOD, sc.d_tok, reps=reps, tail=tail)


#         form            mode  SHERF_EXPERIMENT  debug  tiles per workgroup step
CAPS = {'fp32':          (0,    0,                0,     1),
        'fp32 unbanded': (0,    0,                1024,  1),
        'fp32 squeezed': (12,   0,                0,     1),
        'fp16 h16':      (16,   0,                0,     4),
        'fp16 h8 ahead': (16,   1024,             0,     2),
        'fp16 h8':       (16,   1536,             0,     2)}


@pytest.mark.parametrize('form', list(CAPS))
def test_forward_grid_caps(form):
    """The smallest count past the form's 16 384 workgroups (+ 37: a ragged last tile): the banded / unbanded grid-stride loop makes a second trip.
    Sample c has the tokens and extras of sample c mod 4096, bit for bit (compared on the device); the first period is checked against float64."""
    mode, word, bits, step = CAPS[form]
    sc, dev = E.scene_on_device('base4096')
    n = 32 * 16384 * step + 37
    tiles_n, tiles = (n + 31) // 32, (n + 31) // 32 + 1
    assert -(-tiles_n // step) > 16384
    reps, tail = divmod(n, PERIOD)
    geom = torch.cat([dev.geom.repeat(reps, 1), dev.geom[:tail]]).contiguous()
    with E.experiment(word), E.debug_bits(bits):
        tokens, extras = dev.forward(n, n, mode, dev.buffers(tiles), geom=geom)
    torch.cuda.synchronize()
    for buf, per_tile in ((tokens, 3072), (extras, 384)):
        b = buf.view(torch.int32)
        period = PERIOD // 32 * per_tile
        assert bool((b[:reps * period].view(reps, period) == b[:period]).all()), (form, 'a period differs from the first')
        assert bool((buf[tiles_n * per_tile:] == E.SENT).all()), form
    t_tok = G.untile_tokens(tokens[reps * PERIOD // 32 * 3072:], 64).reshape(64, 96)
    t_ex = G.untile_extras(extras[reps * PERIOD // 32 * 384:], 64)
    assert tail == 37 and bool((t_tok[tail:] == 0).all()) and bool((t_ex[tail:] == 0).all()), form
    assert torch.equal(t_tok[:tail].view(torch.int32), G.untile_tokens(tokens, tail).reshape(tail, 96).view(torch.int32)), form
    assert torch.equal(t_ex[:tail].contiguous().view(torch.int32), G.untile_extras(extras, tail).contiguous().view(torch.int32)), form
    first = (tokens[:PERIOD // 32 * 3072].clone(), extras[:PERIOD // 32 * 384].clone())
    del tokens, extras
    E.assert_forward(sc, f'caps {form} n={n}', first, PERIOD, PERIOD // 32, bool(mode & 16))
