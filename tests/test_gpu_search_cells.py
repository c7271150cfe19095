"""The candidate search by sub-cell on the device: the cases of tests/test_hipcpu_search_cells.py (tests/search_cells_common.py) through the library."""
import pytest
import torch

from sherf_amd import _lib
from tests import search_cells_common as C

gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize('S', C.S_VALUES)
@pytest.mark.parametrize('name', list(C.CASES))
def test_search_by_sub_cell(name, S):
    lib = _lib.lib()
    try:
        C.run_case(lib, lambda v: lib.sherf_set_debug(int(v)), torch.device('cuda', 0), name, S, sync=torch.cuda.synchronize)
    finally:
        lib.sherf_set_debug(0)
