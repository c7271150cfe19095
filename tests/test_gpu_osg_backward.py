"""The backward of the OSGDecoder path (use_NeRF_decoder=False) on the MI355X: the `check_*` bodies of tests/test_hipcpu_osg_backward.py (which runs them
on the host build), here against libsherf_hip.so / libsherf_hip_bwd.so on the device.  The `tiny_ri` frame (628 valid samples) and kernel inputs of at
most 1000 samples only."""
import pytest
import torch

from tests import test_hipcpu_osg_backward as B

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]


def test_osg_head_kernel_against_float64_autograd():
    B.check_head_kernel()


def test_osg_head_abi():
    B.check_head_abi()


@pytest.mark.parametrize('tag', list(B.CASES))
def test_osg_training_step_against_reference_gradients(tag):
    B.check_full_backward(tag)


def test_osg_autograd_switch():
    B.check_switch()
