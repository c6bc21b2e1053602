"""The split kernel's per-set sample order (flux_amd/csrc/flux_sample_order.h) restated in numpy, independently of the header: the key,
the stable sort and the deal.  tests/test_sample_order.py holds the header (compiled for the host) to it, tests/test_gpu_sample_order.py
the device's table."""
import numpy as np

GROUP, QUARTERS = 64, 4


def cell(v):
    """[-1, 1] -> 0 .. 127; NaN, -inf and <= -1 -> 0; +inf and >= 1 - 1/64 -> 127."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (v + 1.0) * 64.0
        out = np.where(s >= 127.0, 127.0, np.where(s > 0.0, np.floor(s), 0.0))  # (a NaN fails both compares)
    return out.astype(np.uint32)


def spread(c):
    c = np.asarray(c, dtype=np.uint32)
    out = np.zeros_like(c)
    for b in range(7):
        out |= ((c >> b) & 1) << (2 * b)
    return out


def key(x, y):
    return spread(cell(x)) | (spread(cell(y)) << 1)


def slice_lo(N, sub, K):
    return N * sub // K


def deal_positions(N):
    """pos[r]: the row position of the r-th element of the sorted sequence.  Element by element: group r // 64 starts at quarter
    (r // 64) % 4; a full quarter hands the element on to the next one."""
    lo = [slice_lo(N, q, QUARTERS) for q in range(QUARTERS + 1)]
    fill = [0] * QUARTERS
    pos = np.empty(N, dtype=np.int64)
    for r in range(N):
        q = (r // GROUP) % QUARTERS
        while fill[q] == lo[q + 1] - lo[q]:
            q = (q + 1) % QUARTERS
        pos[r] = lo[q] + fill[q]
        fill[q] += 1
    return pos


_POS = {}


def row_from_keys(keys):
    keys = np.asarray(keys)
    N = len(keys)
    if N not in _POS:
        _POS[N] = deal_positions(N)
    row = np.empty(N, dtype=np.int64)
    row[_POS[N]] = np.argsort(keys, kind="stable")
    return row


def row_from_hemi(hemi0):
    """hemi0: [N][3], depth row 0 of one set's hemi table."""
    return row_from_keys(key(hemi0[:, 0], hemi0[:, 1]))
