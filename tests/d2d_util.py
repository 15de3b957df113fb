"""Shared by test_gpu_d2d.py and test_gpu_readv.py: inputs, a device arena with guard bytes, and
raw (status-returning) calls of the host-buffer and device-resident decode entry points."""
import ctypes as C

import numpy as np

import bmh
from bmh import synth

GUARD = 0xA5
U64 = 2**64 - 1


N_MAX = 70_000
_text = None


def make_input(kind: str, n: int) -> np.ndarray:
    """The first n <= N_MAX bytes of the Zipf text stream (computed once), or seeded random bytes."""
    global _text
    if kind == "text":
        if _text is None:
            _text = synth.zipf_text(N_MAX)
        return _text[:n].copy()
    return np.random.default_rng(1000 + n).integers(0, 256, n, dtype=np.uint8)


def bound(n: int, bs: int, checksum: bool) -> int:
    L = bmh.lib()
    return int((L.bmh_compress_bound_checked if checksum else L.bmh_compress_bound)(n, bs))


class Arena:
    """One device allocation, refilled with GUARD before a test writes into a window of it."""

    def __init__(self, ctx, nbytes: int):
        self.ctx, self.nbytes = ctx, nbytes
        self.buf = ctx.alloc(nbytes)
        self.base = self.buf.ptr.value
        assert self.base % 256 == 0

    def fill(self) -> None:
        self.buf.upload(np.full(self.nbytes, GUARD, np.uint8))

    def put(self, data, offset: int = 0) -> int:
        self.buf.upload(bmh.as_u8(data), offset)
        return self.base + offset

    def get(self, offset: int = 0, nbytes=None) -> np.ndarray:
        return self.buf.download(nbytes, offset)

    def free(self) -> None:
        self.buf.free()


def raw_decompress_dev(ctx, data: bytes, cap=None):
    """(status, n_out, bytes or None) of bmh_decompress_dev; cap None: the size query."""
    a = bmh.as_u8(data)
    n = C.c_uint64(0xDEAD)
    out = None if cap is None else np.zeros(max(cap, 1), np.uint8)
    st = bmh.lib().bmh_decompress_dev(ctx.h, C.c_void_p(a.ctypes.data), a.size,
                                      None if out is None else C.c_void_p(out.ctypes.data), cap or 0, C.byref(n))
    return st, n.value, (out[:n.value].tobytes() if st == 0 and out is not None else None)


def raw_decompress_d2d(ctx, d_in: int, length: int, d_out=None, cap=None):
    """(status, n_out) of bmh_decompress_d2d on device addresses; cap None: the size query."""
    n = C.c_uint64(0xDEAD)
    st = bmh.lib().bmh_decompress_d2d(ctx.h, C.c_void_p(d_in), length, None if cap is None else C.c_void_p(d_out),
                                      cap or 0, C.byref(n))
    return st, n.value


def raw_verify(ctx, where, length=None):
    """(status, n_out, bad_block) of bmh_verify_dev (where: bytes) or bmh_verify_d2d (where: a
    device address, with length)."""
    n, bad = C.c_uint64(0xDEAD), C.c_uint64(0xBEEF)
    if length is None:
        a = bmh.as_u8(where)
        st = bmh.lib().bmh_verify_dev(ctx.h, C.c_void_p(a.ctypes.data), a.size, C.byref(n), C.byref(bad))
    else:
        st = bmh.lib().bmh_verify_d2d(ctx.h, C.c_void_p(where), length, C.byref(n), C.byref(bad))
    return st, n.value, bad.value
