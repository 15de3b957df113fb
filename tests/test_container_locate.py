"""CPU: the host-only side of the device-resident container calls.

- libbmh.so exports the new entry points and include/bmh.h declares them;
- bmh_container_locate against a brute-force restatement of the geometry rule (block b holds
  plain bytes [b*block_size, min((b+1)*block_size, total_n)), nblocks == ceil(total_n /
  block_size)) with pread clipping, on every block edge and at the ends of the u64 range;
- bmh_container_block_size on hand-built containers around golden records, and on a bare record.
"""
import os
import re
import subprocess

import pytest

import bmh
from crc32_util import build_v1, build_v2
from oracle_ffi import golden_small

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "bmh.h")
NEW = ["bmh_compress_d2d", "bmh_decompress_d2d", "bmh_verify_d2d", "bmh_readv_d2d", "bmh_container_block_size",
       "bmh_container_locate"]
U64 = 2**64 - 1
TOTALS = [1, 2, 4095, 4096, 4097, 70_000]


def test_new_symbols_are_declared_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(bmh_[a-z0-9_]+)\s*\(", txt))
    assert set(NEW) <= declared
    lib = bmh.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True).stdout
    assert set(NEW) <= set(re.findall(r" T (bmh_\w+)", out))
    for n in NEW:
        assert n in bmh._SIGS and hasattr(lib, n)


def _block_sizes(total):
    return sorted({bs for bs in (1, 16, 4096, total - 1, total, total + 1) if 1 <= bs < 2**32 - 1})


def _brute(bs, total, offset, count):
    """(first_block, block_count, skip, n_read) from the rule itself: the blocks whose byte
    interval meets [offset, offset + n_read)."""
    n_read = min(count, total - offset) if offset < total else 0
    if n_read == 0:
        return None, 0, None, 0
    nb = -(-total // bs)
    # (candidates: a window that is one block wider at both ends than any answer can be)
    cand = range(max(0, offset // bs - 1), min(nb, (offset + n_read) // bs + 2))
    touched = [b for b in cand if b * bs < offset + n_read and min((b + 1) * bs, total) > offset]
    assert touched == list(range(touched[0], touched[-1] + 1))
    return touched[0], len(touched), offset - touched[0] * bs, n_read


def _offsets(bs, total):
    """Every block edge and its two neighbours (of the first, last and middle blocks only where
    there are more than 300 blocks), total_n, total_n + 1 and 2^64 - 1."""
    nb = -(-total // bs)
    blocks = range(nb) if nb <= 300 else sorted(set(range(3)) | set(range(nb - 3, nb)) | {nb // 2})
    v = {0, 1, total - 1, total, total + 1, U64}
    for b in blocks:
        for e in (b * bs, min((b + 1) * bs, total)):
            v |= {e - 1, e, e + 1}
    return sorted(x for x in v if 0 <= x <= U64)


def _counts(bs, total, off):
    """Counts that end the read on the next two block edges, on the stream's end and on the
    last block's start, each one short and one past; 0, 1 and the largest values."""
    v = {0, 1, 2, U64, U64 - off, U64 - off + 1}
    ends = [(off // bs + k) * bs for k in (1, 2)] + [total, (total - 1) // bs * bs]
    for e in ends:
        v |= {e - off - 1, e - off, e - off + 1}
    return sorted(c for c in v if 0 <= c <= U64)


@pytest.mark.parametrize("total", TOTALS)
def test_locate_against_brute_force(total):
    checked = 0
    for bs in _block_sizes(total):
        nb = -(-total // bs)
        for off in _offsets(bs, total):
            for cnt in _counts(bs, total, off):
                first, bc, skip, nr = bmh.container_locate(bs, nb, total, off, cnt)
                wf, wbc, ws, wnr = _brute(bs, total, off, cnt)
                assert (bc, nr) == (wbc, wnr), (bs, total, off, cnt)
                if nr:
                    assert (first, skip) == (wf, ws), (bs, total, off, cnt)
                    assert first == off // bs and skip == off - first * bs
                checked += 1
    assert checked > 100


def test_locate_count_and_offset_do_not_wrap():
    # offset + count passes 2^64 - 1: the read is clipped, not wrapped to a small one
    assert bmh.container_locate(4096, 18, 70_000, 69_999, U64) == (17, 1, 69_999 - 17 * 4096, 1)
    assert bmh.container_locate(4096, 18, 70_000, 0, U64) == (0, 18, 0, 70_000)
    assert bmh.container_locate(4096, 18, 70_000, 4095, U64 - 4094) == (0, 18, 4095, 70_000 - 4095)
    for off in (70_000, 70_001, U64):
        assert bmh.container_locate(4096, 18, 70_000, off, U64)[1::2] == (0, 0)
        assert bmh.container_locate(4096, 18, 70_000, off, 1)[1::2] == (0, 0)


def test_locate_count_zero():
    for off in (0, 1, 4095, 4096, 69_999, 70_000):
        assert bmh.container_locate(4096, 18, 70_000, off, 0)[1::2] == (0, 0)


@pytest.mark.parametrize("bs,nb,total", [
    (4096, 17, 70_000), (4096, 19, 70_000),  # nblocks off by one
    (4096, 1, 4097), (4096, 2, 4096), (1, 0, 1), (16, 1, 0),
    (0, 18, 70_000), (0, 0, 0),              # block_size 0
    (2**32 - 1, 1, 5), (2**32 - 1, 1, 2**32 - 1), (2**32, 1, 5),
])
def test_locate_rejects_inconsistent_geometry(bs, nb, total):
    for off, cnt in ((0, 1), (0, 0), (total, 5)):
        with pytest.raises(bmh.BmhError) as e:
            bmh.container_locate(bs, nb, total, off, cnt)
        assert e.value.status == bmh.BMH_ECORRUPT
    # the largest block size the format allows passes
    assert bmh.container_locate(2**32 - 2, 1, 5, 1, 9) == (0, 1, 1, 4)


def test_container_block_size():
    name, data, rec = next(iter(golden_small()))
    for bs in (len(data), 4096, 2**32 - 2):
        assert bmh.container_block_size(build_v1(bs, [data], [rec])) == bs
        assert bmh.container_block_size(build_v2(bs, [data, data], [rec, rec])) == bs
    for bad in (rec, rec[:7], build_v1(7, [data], [rec])[:31], b""):
        with pytest.raises(bmh.BmhError) as e:
            bmh.container_block_size(bad)
        assert e.value.status == bmh.BMH_EINVAL
