"""Reads longer than -l classified over windows (`--windows`): the window rule in numpy, for the host side of the run (argument
checks before anything touches a device, the shard bounds of the label gather, the summary's totals). The device side is
csrc/rd_windows.hpp behind the C ABI rd_window_plan / rd_window_fill / rd_window_fuse; include/ribodetector_amd.h states the rule.

L = -l, S = the stride (1..2^31-1, default L), K = the most windows per read (1..4096, default 32). A read of len bases has W = 1 window
when len <= L - the read itself, classified as ever - and otherwise W = min(K, ceil((len - L) / S) + 1) windows of L bases, window j
starting (j (len - L)) // (W - 1) bases in: the first at the read's start, the last at its end, the others evenly between."""
import numpy as np

from . import _native as N

STRIDE_MAX = (1 << 31) - 1
DEFAULT_MAX_WINDOWS = 32


def check_params(max_len, stride=None, max_windows=DEFAULT_MAX_WINDOWS):
    """(stride, max_windows) as integers, stride None = max_len; RuntimeError for values outside the rule's ranges"""
    stride = int(max_len) if stride is None else int(stride)
    max_windows = int(max_windows)
    if not 1 <= stride <= STRIDE_MAX:
        raise RuntimeError("windows: the stride must be in [1, 2^31 - 1]; got %d" % stride)
    if not 1 <= max_windows <= N.WINDOW_MAX:
        raise RuntimeError("windows: the most windows per read must be in [1, %d]; got %d" % (N.WINDOW_MAX, max_windows))
    return stride, max_windows


def counts(lens, max_len, stride, max_windows):
    """W of every read: int64 array like lens"""
    lens = np.asarray(lens, dtype=np.int64)
    over = np.maximum(lens - int(max_len), 0)
    w = np.minimum((over + (int(stride) - 1)) // int(stride) + 1, int(max_windows))
    return np.where(lens <= int(max_len), 1, w).astype(np.int64)


def starts(length, max_len, w):
    """starts of the w > 1 windows of a read of `length` bases, in bases from its start (Python integers: no overflow)"""
    return [j * (int(length) - int(max_len)) // (int(w) - 1) for j in range(int(w))]
