"""Shared by test_crc32_host.py and test_crc32_gpu.py: BMH containers built by hand in Python
(independent of the encoder) and the mutations the integrity tests apply to them."""
import struct
import zlib

MAGIC1 = b"\xffBMHBLK1"
MAGIC2 = b"\xffBMHBLK2"


def build_v1(block_size: int, datas: list, recs: list) -> bytes:
    return (MAGIC1 + struct.pack("<QQQ", block_size, len(recs), sum(map(len, datas))) +
            b"".join(struct.pack("<Q", len(r)) for r in recs) + b"".join(recs))


def table_bytes_v2(nb: int) -> int:
    """Header, record lengths, CRCs and the zero padding to a multiple of 8."""
    return 32 + 8 * nb + (4 * nb + 7) // 8 * 8


def build_v2(block_size: int, datas: list, recs: list, crcs=None) -> bytes:
    crcs = [zlib.crc32(d) for d in datas] if crcs is None else crcs
    head = (MAGIC2 + struct.pack("<QQQ", block_size, len(recs), sum(map(len, datas))) +
            b"".join(struct.pack("<Q", len(r)) for r in recs) + b"".join(struct.pack("<I", c) for c in crcs))
    head += b"\0" * (-len(head) % 8)
    assert len(head) == table_bytes_v2(len(recs))
    return head + b"".join(recs)


def flip_leaf_bit(rec: bytes) -> bytes:
    """The record with the lowest symbol bit of the first leaf of its preorder tree flipped: the
    tree bits start at byte 24, MSB first; the first 0 bit opens a leaf and its 8 symbol bits
    follow, so the bit 8 positions later is that symbol's lowest bit. The record stays well
    formed and decodes, to other bytes."""
    r = bytearray(rec)
    p = 0
    while (r[24 + p // 8] >> (7 - p % 8)) & 1:
        p += 1
    p += 8
    r[24 + p // 8] ^= 1 << (7 - p % 8)
    return bytes(r)


def record_offset(container: bytes, b: int) -> int:
    """Offset of record b inside a hand-built or encoder-built container of either version."""
    nb = struct.unpack_from("<Q", container, 16)[0]
    o = table_bytes_v2(nb) if container[:8] == MAGIC2 else 32 + 8 * nb
    return o + sum(struct.unpack_from("<Q", container, 32 + 8 * k)[0] for k in range(b))


def crc_offset(container: bytes, b: int) -> int:
    nb = struct.unpack_from("<Q", container, 16)[0]
    return 32 + 8 * nb + 4 * b


def flip_bit(data: bytes, offset: int, bit: int = 0) -> bytes:
    r = bytearray(data)
    r[offset] ^= 1 << bit
    return bytes(r)
