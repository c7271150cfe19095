"""The OSGDecoder path (use_NeRF_decoder=False) on the MI355X: the `check_*` bodies of tests/test_hipcpu_osg.py (which runs them on the host build),
here against libsherf_hip.so on the device.  The `tiny_ri` frame (628 valid samples: three workgroups of the kernel) and 128-sample kernel inputs only."""
import pytest
import torch

from tests import test_hipcpu_osg as OSG

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]


def test_osg_kernel_against_float64():
    OSG.check_kernel()


@pytest.mark.parametrize('tag', list(OSG.CASES))
def test_osg_frame_against_reference_golden(tag):
    OSG.check_frame(tag)


def test_osg_completion_runs_without_transformer():
    OSG.check_completion_without_transformer()


def test_osg_leaves_no_state_behind():
    OSG.check_no_state_left_behind()


def test_osg_construction_and_names():
    OSG.check_construction()


def test_osg_abi():
    OSG.check_abi()
