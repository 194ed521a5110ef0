"""One flat device buffer that every array of a kernel call is carved out of, with guards.

The buffer is filled with a sentinel byte; each array sits at a chosen offset from a 16-byte
boundary with at least GUARD bytes (8 elements of the widest type used, int64) of sentinel before
and after it. ``check()`` downloads the whole buffer and compares it bytewise with the host image:
every guard and every array not declared an output must be unchanged. As a float32 the sentinel is
-4.3e8 and as an integer it is negative, so a kernel that reads a guard shows in its result too.
"""
import numpy as np
import torch

GUARD = 64
SENTINEL = 0xCD


class Arena:
    def __init__(self):
        self._items = {}   # name -> (byte offset, dtype, length, is an output)
        self._size = 0
        self._image = None
        self._buf = None
        self._pending = []

    def add(self, name, array, off16=0, out=False):
        """Places a copy of ``array`` (1-D) ``off16`` bytes past a 16-byte boundary."""
        assert self._buf is None and name not in self._items and 0 <= off16 < 16
        array = np.ascontiguousarray(array).reshape(-1)
        start = -(-(self._size + GUARD) // 16) * 16 + off16
        self._items[name] = (start, array.dtype, array.size, out)
        self._pending.append((start, array.copy()))
        self._size = start + array.nbytes
        return self

    def upload(self, dev):
        size = -(-(self._size + GUARD) // 16) * 16
        self._image = np.full(size, SENTINEL, dtype=np.uint8)
        for start, array in self._pending:
            self._image[start:start + array.nbytes] = array.view(np.uint8)
        self._buf = torch.from_numpy(self._image.copy()).to(dev)
        assert self._buf.data_ptr() % 16 == 0
        return self

    def ptr(self, name, byte_shift=0):
        return self._buf.data_ptr() + self._items[name][0] + byte_shift

    def write(self, name, array):
        """Replaces an array's contents (the next call's input) in the image and on the device."""
        start, dtype, size, _ = self._items[name]
        array = np.ascontiguousarray(array, dtype=dtype).reshape(-1)
        assert array.size == size
        self._image[start:start + array.nbytes] = array.view(np.uint8)
        self._buf[start:start + array.nbytes].copy_(torch.from_numpy(array.view(np.uint8).copy()))

    def check(self, what=""):
        """Synchronises, asserts that everything but the outputs is bytewise the image, and
        returns the outputs {name: array}. An output's new contents become part of the image
        (an in-place kernel's next call starts from them)."""
        got = self._buf.cpu().numpy()
        outs = {}
        masked = got.copy()
        for name, (start, dtype, size, out) in self._items.items():
            if out:
                nbytes = size * np.dtype(dtype).itemsize
                outs[name] = got[start:start + nbytes].copy().view(dtype)
                masked[start:start + nbytes] = self._image[start:start + nbytes]
        if not np.array_equal(masked, self._image):
            at = int(np.flatnonzero(masked != self._image)[0])
            owner = [n for n, (s, d, k, _) in self._items.items()
                     if s <= at < s + k * np.dtype(d).itemsize]
            raise AssertionError(f"{what}: byte {at} changed "
                                 f"({'input ' + owner[0] if owner else 'a guard'})")
        for name, (start, dtype, size, out) in self._items.items():
            if out:
                self._image[start:start + outs[name].nbytes] = outs[name].view(np.uint8)
        return outs


def bits(x):
    """uint32 view of float32 values: equality of these is bitwise equality (signed zeros too)."""
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float32
    return x.view(np.uint32)
