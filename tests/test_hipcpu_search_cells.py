"""The candidate search by sub-cell (csrc/sample.hip: cand_mark_kernel<., true>, cand_cells_alloc_kernel, cand_place_kernel, cand_search_cells_kernel) on the
host build of its source: bit-identical to the search by candidate it replaces and equal to brute force, on the edge geometries of
tests/search_cells_common.py."""
import ctypes

import pytest
import torch

from sherf_amd import _lib
from tests import search_cells_common as C
from tests.hipcpu import build_cpu


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    path = build_cpu.build('sherf_hipcpu_search_cells', ['sample.hip'], str(tmp_path_factory.mktemp('hipcpu_search_cells')),
                           extra_src='char g_sherf_err[256] = ""; int g_sherf_debug = 0;\n')
    return C.bind(ctypes.CDLL(path), _lib.parse_header())


@pytest.mark.parametrize('S', C.S_VALUES)
@pytest.mark.parametrize('name', list(C.CASES))
def test_search_by_sub_cell(lib, name, S):
    dbg = ctypes.c_int.in_dll(lib, 'g_sherf_debug')

    def set_debug(v):
        dbg.value = v
    C.run_case(lib, set_debug, torch.device('cpu'), name, S)
