"""csrc/sample.hip on edge geometry, on the MI355X: the `check_*` bodies of tests/test_hipcpu_sampler_edges.py (which runs them on the host build), here
against libsherf_hip.so on the device with real waves -- ballots, shuffles, the 64-bit LDS atomicMin of the one-wave kernel, persistent grids sized by
the CU count -- and the case only a device of this size reaches: warp_geom_kernel's default grid past its cap of 8192 workgroups (2.1 M samples), on a
PERIODIC input (a base of 4096 queries, checked against brute force on its own, repeated), so that the comparison of the periods stays on the device."""
import pytest
import torch

from tests import test_hipcpu_sampler_edges as E

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]

PERIOD = 4096


@pytest.mark.parametrize('name', E.CELL_SCENES + ('most',))
def test_cell_lists(name):
    E.check_cells(name)


@pytest.mark.parametrize('name', E.RAY_SCENES + ('most',))
def test_scene(name):
    E.check_sampler(name, forms=E.BIG_FORMS)
    E.check_halo_cells(name)


@pytest.mark.parametrize('S', E.S_CASES)
def test_samples_per_ray(S):
    E.check_shape_S(S)


@pytest.mark.parametrize('R', E.R_CASES)
def test_ray_counts(R):
    E.check_shape_R(R)


@pytest.mark.parametrize('S', E.FORM_S)
def test_forms(S):
    E.check_forms('body', S)
    if S == E.S0:
        E.check_halo_cells('body')


def test_ties():
    E.check_ties()
    E.check_forms('flat', E.S0)


def test_capacity():
    E.check_capacity()


def test_nothing_valid():
    E.check_nothing_valid()


@pytest.mark.parametrize('name', ('body', 'wide', 'long', 'flat'))
def test_warp(name):
    E.check_warp(name)


def test_warp_persistent_trips():
    E.check_warp_persistent_trips()


def test_refusals():
    E.check_refusals()


def test_warp_grid_cap():
    """nv = 8192 * 256 + 37: the default grid is capped at 8192 workgroups, so workgroups 0 and 1 make a second trip (the last one ragged).  Query c is
    query c mod 4096: every period equals the first (compared on the device); the first period and the tail are checked against brute force."""
    gr, Q = E.grid('body'), E.build_queries('body', nq=PERIOD)
    nv = 8192 * 256 + 37
    assert min(8192, -(-nv // 256)) == 8192 and -(-nv // (8192 * 256)) == 2
    geom, tvid = E.run_warp(gr, Q, nv=nv)
    reps, tail = divmod(nv, PERIOD)
    assert tail == 37
    assert bool((tvid[:reps * PERIOD].view(reps, PERIOD) == tvid[:PERIOD]).all()), 'a period of cs_tvid differs from the first'
    gb = geom.view(torch.int32)
    assert bool((gb[:reps * PERIOD].view(reps, PERIOD * 8) == gb[:PERIOD].reshape(-1)).all()), 'a period of geom differs from the first'
    guard = (torch.full((E.GUARD, 8), E.FSENT, device=geom.device), torch.full((E.GUARD,), E.SENT, dtype=torch.int32, device=tvid.device))
    E.assert_warp('first period', Q, torch.cat([geom[:PERIOD], guard[0]]), torch.cat([tvid[:PERIOD], guard[1]]))
    E.assert_warp('tail', Q, geom[reps * PERIOD:], tvid[reps * PERIOD:])
