"""Child process of tests/test_hipcpu_gather_edges.py::test_records_are_read_inside_their_array: the gather's forms on the host build of the unchanged
kernel sources, with the occupancy records of every voxel level placed between inaccessible pages (guarded_copy).  Exits 0 and prints a line when no
form read outside them; a read outside ends this process with a signal, which the parent reports."""
import ctypes
import tempfile

from sherf_amd import _lib
from sherf_amd.build import SOURCES
from tests import gpu_common as G
from tests.hipcpu import build_cpu


def main():
    _lib.LIB_PATH = build_cpu.build('sherf_hipcpu_full', SOURCES, tempfile.mkdtemp(prefix='hipcpu_full'), compiler=build_cpu.CLANG)
    _lib._lib = None
    _lib.ptr = lambda t, dtype=None, channels_last_ok=False: None if t is None else ctypes.c_void_p(t.data_ptr())
    _lib.addr = lambda t, dtype=None: None if t is None else t.data_ptr()
    _lib.stream = lambda: ctypes.c_void_p(0)
    G.CPU_SHIM = True
    from tests import test_hipcpu_gather_edges as E
    E.check_records_are_read_inside_their_array()
    print('records stayed inside')


if __name__ == '__main__':
    main()
