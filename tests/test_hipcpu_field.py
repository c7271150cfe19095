"""The field query on the HOST build of the unchanged kernel sources (tests/hipcpu): the bodies of tests/test_gpu_field.py, which runs them on the MI355X,
through the same Python path and the same native driver (csrc/field.hip, csrc/frame.hip: sherf_query_field)."""
import pytest

from tests import test_gpu_field as F
from tests.test_hipcpu_frame import cpu_product          # noqa: F401  (the host builds behind sherf_amd._lib, CPU tensors)


@pytest.mark.parametrize('case', list(F.CASES))
def test_query_matches_the_reference_goldens(cpu_product, case):
    F.check_reference_golden(case)


@pytest.mark.parametrize('prec', ['f16x3', 'bf16'])
def test_query_has_the_frames_bits(cpu_product, prec):
    F.check_same_bits_as_frame(prec)


def test_query_through_the_dense_marcher_gives_the_golden_image(cpu_product):
    F.check_through_the_marcher()


def test_per_point_indexing(cpu_product):
    F.check_per_point_indexing()


def test_edge_shapes_chunks_and_token_resize(cpu_product):
    F.check_edge_shapes()


def test_frames_around_a_query_are_undisturbed(cpu_product):
    F.check_neighbours_undisturbed()


def test_abi_rejects_bad_arguments(cpu_product):
    F.check_abi_rejects_bad_arguments()


def test_scatter_alone_overflow_and_guard_words(cpu_product):
    F.check_scatter_alone()


def test_generator_sample_and_density_grid(cpu_product):
    F.check_generator()
