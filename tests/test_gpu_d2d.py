"""GPU: the device-resident container calls (bmh_compress_d2d, bmh_decompress_d2d, bmh_verify_d2d).

The references are existing code: compress_d2d must write the bytes of the host path
(Context.compress_bytes), decompress_d2d / verify_d2d must answer as bmh_decompress_dev /
bmh_verify_dev do on the same bytes, damaged ones included."""
import os
import struct

import numpy as np
import pytest

import bmh
from crc32_util import crc_offset, flip_bit, table_bytes_v2
from d2d_util import GUARD, Arena, bound, make_input, raw_decompress_d2d, raw_decompress_dev, raw_verify
from oracle_ffi import GOLDEN

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 255, 4097, 70_000]
IN_AT, OUT_AT, ARENA = 0, 1 << 20, 4 << 20  # input window, output window (8-byte aligned), arena bytes


def block_sizes(n):
    return sorted({bs for bs in (0, 16, 4096, n - 1, n, n + 1) if bs >= 0})


CASES = [(kind, n, bs, ck) for kind in ("text", "random") for n in SIZES for bs in block_sizes(n) for ck in (False, True)]
CASES.append(("text", 300, 1, False))  # 300 one-byte blocks: an even CRC table ...
CASES.append(("text", 300, 1, True))
CASES.append(("text", 299, 1, True))   # ... and an odd one, padded
PAIRS = sorted({c[:2] for c in CASES})


@pytest.fixture(scope="module")
def arena(ctx):
    a = Arena(ctx, ARENA)
    yield a
    a.free()


_ref = {}


def reference(ctx, kind, n, bs, ck):
    """(input, the host path's output) of a case, computed once."""
    key = (kind, n, bs, ck)
    if key not in _ref:
        data = make_input(kind, n)
        _ref[key] = (data, ctx.compress_bytes(data, bs, checksum=ck))
    return _ref[key]


def d2d(ctx, arena, data, bs, ck, cap=None):
    d_in = arena.put(data, IN_AT)
    cap = bound(data.size, bs, ck) if cap is None else cap
    assert OUT_AT + cap <= ARENA and data.size <= OUT_AT
    n = ctx.compress_d2d(d_in, data.size, bs, arena.base + OUT_AT, cap, checksum=ck)
    return arena.get(OUT_AT, n).tobytes()


@pytest.mark.parametrize("kind,n", PAIRS)
def test_compress_d2d_is_byte_identical_to_the_host_path(ctx, arena, kind, n):
    for _, _, bs, ck in [c for c in CASES if c[:2] == (kind, n)]:
        data, want = reference(ctx, kind, n, bs, ck)
        got = d2d(ctx, arena, data, bs, ck)
        assert got == want, (kind, n, bs, ck, len(got), len(want))
        one_block = bs == 0 or bs >= n
        assert bmh.container_version(got) == (2 if ck else 0 if one_block else 1)


def test_compress_d2d_golden_calgary_single_block(ctx, arena):
    with open(os.path.join(GOLDEN, "calgary", "bib"), "rb") as f:
        bib = np.frombuffer(f.read(), np.uint8)
    with open(os.path.join(GOLDEN, "calgary_records", "bib.bzap"), "rb") as f:
        gold = f.read()
    assert d2d(ctx, arena, bib, 0, False) == gold


def test_compress_d2d_small_device_batches(ctx, arena):
    """9 device batches of two 4 KiB blocks: from the second on, a batch's first record starts
    wherever the previous batch's records ended."""
    try:
        ctx.set_option("max_batch", 8192)
        for ck in (False, True):
            data, want = reference(ctx, "text", 70_000, 4096, ck)
            assert d2d(ctx, arena, data, 4096, ck) == want
        ends = np.cumsum(np.frombuffer(want, "<u8", 18, 32))[1::2]  # where batches 0..8 end, from the table
        assert any(int(e) % 4 for e in ends[:-1])  # a later batch did start off a word boundary
    finally:
        ctx.set_option("max_batch", 0)


def _raises(status, fn, *a, **kw):
    with pytest.raises(bmh.BmhError) as e:
        fn(*a, **kw)
    assert e.value.status == status, str(e.value)


@pytest.mark.parametrize("ck", [False, True])
def test_compress_d2d_capacity_and_guards(ctx, arena, ck):
    data, want = reference(ctx, "text", 70_000, 4096, ck)
    L, n = len(want), data.size
    d_in, d_out = arena.base + IN_AT, arena.base + OUT_AT

    def guard_intact(cap):
        a = arena.get()
        return bool((a[n:OUT_AT] == GUARD).all() and (a[OUT_AT + cap:] == GUARD).all())

    arena.fill()
    assert d2d(ctx, arena, data, 4096, ck, cap=L) == want  # the exact length is enough
    assert guard_intact(L)
    table = table_bytes_v2(18) if ck else 32 + 8 * 18
    for cap in (L - 1, table, table - 8, 0):
        arena.fill()
        arena.put(data, IN_AT)
        _raises(bmh.BMH_ERANGE, ctx.compress_d2d, d_in, n, 4096, d_out, cap, checksum=ck)
        assert guard_intact(cap), cap
    arena.fill()
    arena.put(data, IN_AT)
    cap = bound(n, 4096, ck)
    _raises(bmh.BMH_EINVAL, ctx.compress_d2d, d_in, n, 4096, d_out + 4, cap, checksum=ck)  # misaligned output
    _raises(bmh.BMH_EINVAL, ctx.compress_d2d, d_in, n, 4096, d_in + n - 8, cap, checksum=ck)  # overlap
    _raises(bmh.BMH_EINVAL, ctx.compress_d2d, d_in + 8, n, 4096, d_in, cap, checksum=ck)
    _raises(bmh.BMH_EINVAL, ctx.compress_d2d, d_in, 0, 4096, d_out, cap, checksum=ck)  # empty input
    _raises(bmh.BMH_EINVAL, ctx.compress_d2d, None, n, 4096, d_out, cap, checksum=ck)
    _raises(bmh.BMH_ERANGE, ctx.compress_d2d, d_in, 2**33, 2**32 - 1, d_out + 2**34, 2**34, checksum=ck)
    assert guard_intact(0)
    assert d2d(ctx, arena, data, 4096, ck) == want  # the context still works


@pytest.mark.parametrize("kind,n", PAIRS)
def test_decompress_d2d_round_trip(ctx, arena, kind, n):
    for _, _, bs, ck in [c for c in CASES if c[:2] == (kind, n)]:
        data, stream = reference(ctx, kind, n, bs, ck)
        for shift in (0, 1):  # the stream at an aligned and at an odd address
            arena.fill()
            d_s = arena.put(stream, IN_AT + shift)
            d_o = arena.base + OUT_AT + 3 * shift
            assert ctx.decompress_d2d(d_s, len(stream)) == n  # the size query
            assert ctx.decompress_d2d(d_s, len(stream), d_o, n) == n
            out = arena.get(OUT_AT - 16, n + 64)
            assert out[16 + 3 * shift:16 + 3 * shift + n].tobytes() == data.tobytes(), (kind, n, bs, ck, shift)
            assert (out[:16 + 3 * shift] == GUARD).all() and (out[16 + 3 * shift + n:] == GUARD).all()
            _raises(bmh.BMH_ERANGE, ctx.decompress_d2d, d_s, len(stream), d_o, n - 1)
            assert ctx.verify_d2d(d_s, len(stream)) == n


def _damaged(v2, v2odd):
    """(name, bytes) of every damage: of the 70 000 / 4096 version-2 container, and of one with
    17 blocks for the CRC table's padding. Each damaged field is one the host side checks before
    it launches anything."""
    def put_len(s, b, v):
        return s[:32 + 8 * b] + struct.pack("<Q", v) + s[40 + 8 * b:]

    table = table_bytes_v2(18)
    assert len(v2odd) > table_bytes_v2(17) and table_bytes_v2(17) == 32 + 12 * 17 + 4
    last = struct.unpack_from("<Q", v2, 32 + 8 * 17)[0]
    return [
        ("intact", v2), ("intact odd", v2odd),
        ("cut 31", v2[:31]), ("cut table-1", v2[:table - 1]), ("cut table+23", v2[:table + 23]),
        ("cut len-1", v2[:-1]),
        ("crc flipped", flip_bit(v2, crc_offset(v2, 7) + 2, 5)),
        ("padding", flip_bit(v2odd, 32 + 12 * 17 + 1, 0)),
        ("record_len overrun", put_len(v2, 17, last + 8)),
        ("record_len huge", put_len(v2, 3, 2**63)),
        ("bad magic", v2[:7] + b"3" + v2[8:]),
        ("empty", b""),
    ]


@pytest.fixture(scope="module")
def damaged(ctx):
    data, v2 = reference(ctx, "text", 70_000, 4096, True)
    v2odd = ctx.compress_bytes(data, 4200, checksum=True)
    assert struct.unpack_from("<Q", v2odd, 16)[0] == 17
    return data, _damaged(v2, v2odd)


def test_damaged_streams_answer_as_the_host_buffer_paths(ctx, arena, damaged):
    data, cases = damaged
    n = data.size
    seen = set()
    for name, s in cases:
        # existing code on the same bytes (an empty stream gets one byte of backing store)
        host = np.frombuffer(s, np.uint8) if s else np.zeros(1, np.uint8)[:0]
        want_q = raw_decompress_dev(ctx, host)
        want_d = raw_decompress_dev(ctx, host, cap=n)
        want_v = raw_verify(ctx, host)
        for shift in (0, 1):
            arena.fill()
            d_s = arena.put(s, IN_AT + shift) if s else arena.base + IN_AT + shift
            d_o = arena.base + OUT_AT
            assert raw_decompress_d2d(ctx, d_s, len(s)) == want_q[:2], name
            got = raw_decompress_d2d(ctx, d_s, len(s), d_o, cap=n)
            assert got == want_d[:2], name
            if got[0] == bmh.BMH_OK:
                assert arena.get(OUT_AT, got[1]).tobytes() == want_d[2] == data.tobytes(), name
            assert (arena.get(OUT_AT + n, 4096) == GUARD).all(), name
            assert raw_verify(ctx, d_s, len(s)) == want_v, name
        seen.add((name.split()[0], want_d[0], want_v[2] != 2**64 - 1))
    # the cases did exercise what they are named for
    assert ("intact", bmh.BMH_OK, False) in seen and ("crc", bmh.BMH_ECORRUPT, True) in seen
    assert all(st == bmh.BMH_ECORRUPT and not bad for nm, st, bad in seen if nm not in ("intact", "crc"))
    # and the context still decodes the good stream
    d_s = arena.put(cases[0][1], IN_AT)
    assert ctx.verify_d2d(d_s, len(cases[0][1])) == n
    with pytest.raises(bmh.BmhError) as e:
        bad = cases[6][1]
        ctx.verify_d2d(arena.put(bad, IN_AT), len(bad))
    assert e.value.status == bmh.BMH_ECORRUPT and e.value.bad_block == 7 and "block 7" in str(e.value)
