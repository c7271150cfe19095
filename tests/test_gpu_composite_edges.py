"""csrc/composite.hip per ray on edge rays, on the MI355X: the `check_*` bodies of tests/test_hipcpu_composite_edges.py (which runs them on the host build), here
against libsherf_hip.so on the device -- real 256-thread blocks, the device's expf / log1pf, atomicOr on the overflow flag from many rays at once -- against
the same fp64 transcription and the same bounds.  No case reads outside a buffer by construction: sample_out / cs_idx hold every row a launch may touch,
and the backward is never given a ray beyond its buffers."""
import pytest
import torch

from tests import test_hipcpu_composite_edges as E

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]


@pytest.mark.parametrize('name', E.CASE_NAMES)
def test_rays(name):
    E.check_case(name)


def test_capacity_boundary():
    E.check_capacity()


def test_every_ray_over_capacity():
    """R = 513 rays in three blocks, every one beyond tok_cap: all NaN, and the flag the rays OR together is 2 (with bit 0 kept), not a sum"""
    E.check_capacity(R_over=513)


def test_refusals():
    E.check_refusals()


def test_backward_refuses_an_overflowed_frame():
    E.check_backward_refuses_an_overflowed_frame()
