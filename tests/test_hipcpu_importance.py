"""Importance sampling on the HOST build of the unchanged kernel sources (tests/hipcpu): the bodies of tests/test_gpu_importance.py, which runs them on the
MI355X, through the same Python path and the same native driver (csrc/importance.hip, csrc/composite.hip, csrc/frame.hip: sherf_render_frame_importance)."""
import pytest

from tests import test_gpu_field as F
from tests import test_gpu_importance as I
from tests.test_hipcpu_frame import cpu_product          # noqa: F401  (the host builds behind sherf_amd._lib, CPU tensors)


@pytest.mark.parametrize('ci', range(6))
def test_resampling_kernel_against_the_reference(cpu_product, ci):
    I.check_resampling(ci)


@pytest.mark.parametrize('ci', range(2))
def test_merged_compositing_alone(cpu_product, ci):
    I.check_merged(ci)


def test_fine_pass_pinned_to_the_reference(cpu_product):
    I.check_fine_pass_pinned()


@pytest.mark.parametrize('case', ['nerf-f16x3', 'nerf-bf16', 'osg', 'f101', 'nerf-f16x3/softplus'])
def test_frame_is_the_staged_composition(cpu_product, case):
    _, decoder, branches, prec = F.CASES[case.split('/')[0]]
    I.check_frame_staged(prec, decoder, branches, 'softplus' if case.endswith('softplus') else 'relu')


def test_frame_against_the_golden_image(cpu_product):
    I.check_frame_against_golden()


def test_seeds_neighbours_and_token_resize(cpu_product):
    I.check_seeds_neighbours_and_resize()


def test_what_raises(cpu_product):
    I.check_raises()


def test_generator_passes_the_option_through(cpu_product):
    I.check_generator()
