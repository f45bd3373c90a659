"""Buffers for calling the C ABI with leading dimensions larger than the row and with room behind the last row -- numpy only
(tests/test_gpu_abi_forms.py puts them on the device; tests/test_abi.py checks the helpers themselves).

Two kinds of padding:

* INPUT padding is NaN: a read past column D or past row M poisons the result visibly;
* OUTPUT padding and tails carry one fixed non-NaN bit pattern (``FILL``): a write past column D, or of the padded row count
  instead of the real one, changes it.  ``untouched`` compares bit patterns (as uint64), so it works for a NaN fill too.
"""
import numpy as np

#: what output padding is filled with: a finite double no computation here produces (about -2.7e-231)
FILL_BITS = np.uint64(0x900DF00DCAFE5A5A)
FILL = np.array([FILL_BITS], dtype=np.uint64).view(np.float64)[0]
#: spare elements behind the last row of every output buffer (at least)
SPARE = 64


def embed(a, ld, fill, spare=SPARE):
    """The 2-D array ``a`` (rows x width) in a C-contiguous buffer of leading dimension ``ld >= width``: ``(rows + extra, ld)``
    with ``a`` in ``[:rows, :width]`` and ``fill`` everywhere else; ``extra`` rows give at least ``spare`` elements behind row
    ``rows - 1``."""
    a = np.asarray(a, dtype=np.float64)
    rows, width = a.shape
    if ld < width:
        raise ValueError(f"ld = {ld} is smaller than the row ({width})")
    extra = -(-int(spare) // int(ld)) if spare > 0 else 0
    buf = np.full((rows + extra, ld), fill, dtype=np.float64)
    buf[:rows, :width] = a
    return buf


def padded(n, extra, fill, values=None):
    """A vector of ``n`` elements (``values``, or ``fill``) followed by a tail of ``extra`` elements of ``fill``."""
    buf = np.full(int(n) + int(extra), fill, dtype=np.float64)
    if values is not None:
        buf[:n] = np.asarray(values, dtype=np.float64)
    return buf


def untouched(buf, width, fill_bits, rows=None):
    """True when every padding element of ``buf`` still carries the fill's exact bit pattern.  2-D ``buf`` (as ``embed`` makes
    it): the columns from ``width`` on in every row and, with ``rows``, every row from ``rows`` on.  1-D ``buf`` (``padded``): the
    elements from ``width`` on."""
    bits = np.ascontiguousarray(buf, dtype=np.float64).view(np.uint64)
    want = np.uint64(fill_bits)
    if bits.ndim == 1:
        return bool(np.all(bits[width:] == want))
    ok = np.all(bits[:, width:] == want)
    if rows is not None:
        ok = ok and np.all(bits[rows:] == want)
    return bool(ok)


def bits_of(fill):
    """The uint64 bit pattern of the float64 ``fill``."""
    return np.array([fill], dtype=np.float64).view(np.uint64)[0]
