"""GPU: the CRC-32 kernels against zlib, the version-2 container through every encode path
(streamed, pinned, multi-context, one block), the check on both GPU decode paths, and the CLI's
`--checksum` / `test` modes."""
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import bmh
from bmh import synth
from crc32_util import crc_offset, flip_bit, flip_leaf_bit, record_offset

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "bwt-mtf-huffman-compressor_amd", "bin", "bmh")
# the kernel's tile: the sizes below sit on and around it
T = int(re.search(r"kCrcTile = (\d+);", open(os.path.join(
    REPO, "bwt-mtf-huffman-compressor_amd", "csrc", "crc32.hip")).read()).group(1))
SIZES = [1, 2, 3, 15, 16, 17, 63, 1023, 1024, 1025, T - 1, T, T + 1, 2 * T + 1, 65537, 262147]
BS = 1 << 20


def _crc_dev(ctx, a: np.ndarray, sizes) -> list:
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    assert int(offs[-1]) == a.size
    d = ctx.alloc(a.size)
    try:
        d.upload(a)
        return [int(x) for x in ctx.crc32_dev(d, offs)]
    finally:
        d.free()


def _zlib(a: np.ndarray, sizes) -> list:
    out, o = [], 0
    for n in sizes:
        out.append(zlib.crc32(a[o:o + n].tobytes()))
        o += n
    return out


@pytest.mark.parametrize("fill", ["zeros", "ones", "random"])
def test_crc32_dev_back_to_back_blocks(ctx, fill):
    """Odd block starts, sizes on and around the 16-byte chunk, the 1 KiB row and the tile. On
    all zeros the CRC depends on the length alone: a wrong length or shift power shows there."""
    total = sum(SIZES)
    a = {"zeros": np.zeros(total, np.uint8), "ones": np.full(total, 0xFF, np.uint8),
         "random": np.random.default_rng(11).integers(0, 256, total, dtype=np.uint8)}[fill]
    assert _crc_dev(ctx, a, SIZES) == _zlib(a, SIZES)
    rev = SIZES[::-1]  # other starts for the same sizes
    assert _crc_dev(ctx, a, rev) == _zlib(a, rev)


def test_crc32_dev_bench_shape_and_long_blocks(ctx):
    # 4 x 4 MiB of splitmix64 bytes generated on the device (the benchmark's block shape)
    n = 4 << 20
    d = ctx.alloc(4 * n)
    try:
        ctx.synth_splitmix64(d, 4 * n, seed=0)
        offs = np.arange(5, dtype=np.uint64) * np.uint64(n)
        got = [int(x) for x in ctx.crc32_dev(d, offs)]
        a = d.download()
    finally:
        d.free()
    assert np.array_equal(a, synth.splitmix64_bytes(0, 0, 4 * n))
    assert got == _zlib(a, [n] * 4)
    # one block whose full tiles do not divide among the fold's 64 lanes (some lanes get two
    # tiles, one gets one, the rest none), then, from an odd start, one of 64 MiB + 1: 4096 full
    # tiles, 64 Horner steps on every lane, and the one-byte last tile
    rng = np.random.default_rng(12)
    sizes = [65 * T + 5, 3, (64 << 20) + 1]
    a = rng.integers(0, 256, sum(sizes), dtype=np.uint8)
    assert _crc_dev(ctx, a, sizes) == _zlib(a, sizes)


@pytest.fixture(scope="module")
def text():
    data = synth.zipf_text(3_000_001)
    blocks = [data[i:i + BS].tobytes() for i in range(0, data.size, BS)]
    assert [len(b) for b in blocks] == [BS, BS, 3_000_001 - 2 * BS]
    return data, blocks


@pytest.fixture(scope="module")
def packed(ctx, text):
    """(v1, v2) of the text at 1 MiB blocks; v1 is taken before the option is ever set."""
    data, _ = text
    v1 = ctx.compress_bytes(data, BS)
    v2 = ctx.compress_bytes(data, BS, checksum=True)
    return v1, v2


def test_v2_container_roundtrip(ctx, text, packed):
    data, blocks = text
    v1, v2 = packed
    assert bmh.container_version(v1) == 1 and bmh.container_version(v2) == 2
    assert bmh.container_records(v2) == bmh.container_records(v1)
    assert bmh.container_crcs(v2) == [zlib.crc32(b) for b in blocks]
    assert len(v2) == len(v1) + 4 * 3 + 4  # the CRC table and its padding
    assert ctx.decompress_bytes(v2) == data.tobytes()
    assert bmh.decompress_bytes(v2) == data.tobytes()
    assert ctx.verify(v2) == data.size
    assert ctx.verify(v1) == data.size and ctx.verify(bmh.container_records(v1)[0]) == BS


def test_v2_multi_context_and_small_batches(ctx, text, packed):
    data, _ = text
    _, v2 = packed
    other = bmh.Context(0)
    try:
        assert bmh.compress_bytes_multi([ctx, other], data, BS, checksum=True) == v2
        for c in (ctx, other):
            c.set_option("stream_batch", BS)  # one block a batch: the three batches use every slot
        assert bmh.compress_bytes_multi([ctx, other], data, BS, checksum=True) == v2
        assert ctx.compress_bytes(data, BS, checksum=True) == v2
    finally:
        ctx.set_option("stream_batch", 0)
        other.close()


def test_v2_pinned_in_and_out(ctx, text, packed):
    data, _ = text
    _, v2 = packed
    cap = int(bmh.lib().bmh_compress_bound_checked(data.size, BS))
    hin, hout = ctx.alloc_host(data.size), ctx.alloc_host(cap)
    try:
        hin.a[:] = data
        ctx.set_option("checksum", 1)
        n = ctx.compress_into(hin.a, BS, hout.a)
        assert hout.a[:n].tobytes() == v2
        # the early capacity check counts the version-2 tables
        small = np.empty(32 + 8 * 3 + 8, np.uint8)
        with pytest.raises(bmh.BmhError) as e:
            ctx.compress_into(hin.a, BS, small)
        assert e.value.status == bmh.BMH_ERANGE
    finally:
        ctx.set_option("checksum", 0)
        hin.free()
        hout.free()


def test_v2_single_block(ctx, text):
    _, blocks = text
    one = ctx.compress_bytes(blocks[2], 0, checksum=True)
    assert bmh.container_version(one) == 2
    assert bmh.container_records(one) == ctx.encode_blocks([blocks[2]])
    assert bmh.container_crcs(one) == [zlib.crc32(blocks[2])]
    assert ctx.decompress_bytes(one) == blocks[2] and ctx.verify(one) == len(blocks[2])
    assert ctx.compress_bytes(blocks[2], 0) == bmh.container_records(one)[0]  # off: the bare record


def test_corruption_is_reported_on_the_gpu_paths(ctx, text, packed):
    data, _ = text
    _, v2 = packed
    # a flipped bit in block 1's stored CRC: the data decodes correctly, only the check can notice
    bad = flip_bit(v2, crc_offset(v2, 1) + 1, 3)
    for fn in (ctx.decompress_bytes, ctx.verify):
        with pytest.raises(bmh.BmhError) as e:
            fn(bad)
        assert e.value.status == bmh.BMH_ECORRUPT
        assert re.search(r"block 1\b", str(e.value)), str(e.value)
    assert e.value.bad_block == 1
    # the leaf-bit mutation of record 1: the LF-cycle check or the CRC reports it
    rec = bmh.container_records(v2)[1]
    o = record_offset(v2, 1)
    assert v2[o:o + len(rec)] == rec
    mut = v2[:o] + flip_leaf_bit(rec) + v2[o + len(rec):]
    for fn in (ctx.decompress_bytes, ctx.verify):
        with pytest.raises(bmh.BmhError) as e:
            fn(mut)
        assert e.value.status == bmh.BMH_ECORRUPT
    # a structural failure names no block
    with pytest.raises(bmh.BmhError) as e:
        ctx.verify(v2[:len(v2) - 1])
    assert e.value.status == bmh.BMH_ECORRUPT and e.value.bad_block is None
    # the context still decodes the good container
    assert ctx.decompress_bytes(v2) == data.tobytes()
    assert ctx.verify(v2) == data.size


def test_option_off_output_is_unchanged(ctx, text, packed):
    data, _ = text
    v1, v2 = packed
    try:
        ctx.set_option("checksum", 1)
        n = np.empty(len(v2), np.uint8)
        assert ctx.compress_into(data, BS, n) == len(v2) and n.tobytes() == v2
        ctx.set_option("checksum", 0)
        assert ctx.compress_bytes(data, BS) == v1
    finally:
        ctx.set_option("checksum", 0)


@pytest.mark.skipif(not os.path.exists(CLI), reason="bin/bmh not built")
def test_cli_checksum_and_test_mode(tmp_path, text, packed):
    data, _ = text
    v1, v2 = packed
    src, enc, dec, bad, plain = (str(tmp_path / x) for x in ("in", "in.bmh", "out", "bad.bmh", "v1.bmh"))
    data.tofile(src)
    with open(plain, "wb") as f:
        f.write(v1)
    r = subprocess.run([CLI, "test", plain], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == f"{plain}: OK, 3 blocks, no checksums", (r.stdout, r.stderr)
    r = subprocess.run([CLI, "compress", src, enc, "--block-size", str(BS), "--checksum"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(enc, "rb").read() == v2
    recs = bmh.container_records(v2)
    header = 32 + 8 * 3 + 16 + sum(24 + int.from_bytes(x[16:24], "little") for x in recs)
    assert r.stdout.startswith(f"header size: {header} $$ ")
    for extra in ([], ["--host"]):
        r = subprocess.run([CLI, "test", enc] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout.strip() == f"{enc}: OK, 3 blocks, CRC-32 verified"
    assert subprocess.run([CLI, "decompress", enc, dec]).returncode == 0
    assert open(dec, "rb").read() == data.tobytes()
    with open(bad, "wb") as f:
        f.write(flip_bit(v2, crc_offset(v2, 2), 0))
    r = subprocess.run([CLI, "test", bad], capture_output=True, text=True)
    assert r.returncode == 2 and "block 2" in r.stderr, (r.returncode, r.stderr)
