"""The LDS d_tf table of the brick backward's main kernel (B1, csrc/march_flat.hip: dtf_slot, dtf_slot_of): the sample loop adds
component q of texel k to element dtf_slot(R, k, 0) + q * stride, the zeroing walks 4 R elements, and the flush hands element
dtf_slot_of(R, g) to entry g = 4 k + q of the caller's [texel][4] table (dtf64_add). The library's host view of those three index
functions (dr_b1_dtf_table_map) must agree for every TF resolution the fast path serves: every (k, q) has an element of its own,
the flush reads exactly the element the adds went to, and no index reaches 4 R -- the table's end, behind which the LDS
allocation ends."""
import ctypes

import numpy as np


def test_add_zero_and_flush_agree_for_every_resolution(hiplib):
    fn = hiplib.dr_b1_dtf_table_map
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    layouts = set()
    for R in range(1, 2031):
        add = np.full(4 * R, -1, np.int32)
        flush = np.full(4 * R, -1, np.int32)
        zeroed = fn(R, add.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), flush.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        assert zeroed == 4 * R, R
        assert add.min() >= 0 and add.max() < zeroed, (R, int(add.min()), int(add.max()))        # the adds stay inside what was zeroed
        assert flush.min() >= 0 and flush.max() < zeroed, (R, int(flush.min()), int(flush.max()))  # ... and so does the flush
        assert np.array_equal(np.sort(add), np.arange(4 * R)), R     # one element per (texel, component): nothing shared, nothing unused
        assert np.array_equal(flush, add), R                         # entry 4 k + q of the caller's table receives what (k, q) added
        if R > 1:
            k = np.arange(4 * R) >> 2
            q = np.arange(4 * R) & 3
            layouts.add("component-major" if np.array_equal(add, q * R + k) else "texel-major" if np.array_equal(add, 4 * k + q) else "other")
    assert len(layouts) == 1 and "other" not in layouts, layouts
