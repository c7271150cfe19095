"""Child process of tests/test_hipcpu_composite_edges.py::test_reads_stay_inside_the_compact_arrays: the compact compositing kernels on the host build of the
unchanged kernel sources, with sample_out and cs_idx ending at an inaccessible page (guarded_copy).  Exits 0 and prints a line when no kernel read behind
them; a read outside ends this process with a signal, which the parent reports."""
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
    from tests import test_hipcpu_composite_edges as E
    E.check_reads_stay_inside()
    print('reads stayed inside')


if __name__ == '__main__':
    main()
