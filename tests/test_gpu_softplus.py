"""clamp_mode='softplus' and the differentiable dense MipRayMarcher2 on the MI355X: the `check_*` bodies of tests/test_hipcpu_softplus.py
(which runs them on the host build), here against libsherf_hip.so on the device.  Tiny configurations and the R = 300, S in {2, 5}
marcher inputs only."""
import pytest
import torch

from tests import test_hipcpu_softplus as SP

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]


def test_dense_marcher_softplus_forward():
    SP.check_dense_forward()


def test_dense_marcher_backward_both_modes():
    SP.check_dense_backward()


def test_rejected_samples_skip_exactly_under_softplus():
    SP.check_rejected_samples_skip_exactly()


def test_frame_under_softplus():
    SP.check_frame()


def test_whole_chain_backward_under_softplus():
    SP.check_whole_chain_backward()


def test_softplus_abi():
    SP.check_abi()
