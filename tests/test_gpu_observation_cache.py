"""Reuse of the encoded observation across the frames of a sweep on the MI355X: the `check_*` bodies of tests/test_hipcpu_observation_cache.py
(which runs them on the host build), here against libsherf_hip.so on the device -- three real streams, frames issued back to back."""
import pytest
import torch

from tests import test_hipcpu_observation_cache as C

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]


@pytest.mark.parametrize('aux', (True, False))
@pytest.mark.parametrize('case', list(C.SWEEPS))
def test_camera_sweep_is_bit_identical(case, aux):
    C.check_camera_sweep(case, aux)


def test_pose_sweep_is_bit_identical():
    C.check_pose_sweep()


@pytest.mark.parametrize('cfg', ['tiny_ri', 'cfg1_ri'])
def test_reused_frame_against_reference_golden(cfg):
    """cfg1_ri (128 x 128 x 32, 256^2 planes): the smallest shape where the encoder and the ray side really overlap."""
    C.check_reused_frame_against_golden(cfg)


def test_every_change_of_the_observation_misses():
    C.check_invalidation()


def test_running_statistics_evolve_as_without_reuse():
    C.check_running_statistics()


def test_grad_recorded_forward_ignores_the_option():
    C.check_autograd_ignores_the_option()


def test_two_phase_frames_reuse():
    C.check_two_phase_frames()


def test_generator_caches_the_observation_side():
    C.check_generator_cache()


def test_observation_abi():
    C.check_abi()
