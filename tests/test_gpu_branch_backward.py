"""Training with a feature branch switched off on the MI355X: the `check_*` bodies of tests/test_hipcpu_branch_backward.py (which runs them on the host
build), here against libsherf_hip.so / libsherf_hip_bwd.so on the device.  The `tiny_ri` frame (628 valid samples) and the synthetic scenes of
tests/test_hipcpu_gather_edges.py only."""
import pytest
import torch

from tests import test_hipcpu_branch_backward as B

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]


@pytest.mark.parametrize('n', (1, 33, 65, 200))
def test_masked_scatter_against_float64(n):
    B.check_masked_scatter(n)


def test_masked_scatter_long_run():
    B.check_masked_scatter_long_run()


def test_masked_scatter_abi():
    B.check_masked_abi()


@pytest.mark.parametrize('tag', list(B.CASES))
def test_branch_training_step_against_reference_gradients(tag):
    B.check_training_step(tag)


def test_running_statistics_follow_the_constructor_switch():
    B.check_running_statistics()


def test_degenerate_switches_train_like_planes_alone():
    B.check_degenerate_switches()


def test_what_a_branch_step_runs():
    B.check_what_runs()
