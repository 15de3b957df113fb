"""GPU: bmh_readv_d2d, the vectored range read of a stream in device memory, and its copy kernel
k_gather_pieces. The reference is the plain text itself: every range must equal its slice."""
import struct

import numpy as np
import pytest

import bmh
from crc32_util import crc_offset, flip_bit
from d2d_util import GUARD, U64, Arena, make_input, raw_decompress_d2d, raw_decompress_dev

pytestmark = pytest.mark.gpu

N, BS, NB = 70_000, 4096, 18  # the last block holds 368 bytes
IN_AT, OUT_AT, ARENA = 0, 1 << 18, 1 << 20


@pytest.fixture(scope="module")
def arena(ctx):
    a = Arena(ctx, ARENA)
    yield a
    a.free()


@pytest.fixture(scope="module")
def streams(ctx):
    """The text and its three streams: version-1 and version-2 containers of 4096-byte blocks,
    and the bare record of the whole text (one block)."""
    text = make_input("text", N)
    s = {"v1": ctx.compress_bytes(text, BS), "v2": ctx.compress_bytes(text, BS, checksum=True),
         "bare": ctx.compress_bytes(text, 0)}
    assert [bmh.container_version(s[k]) for k in ("v1", "v2", "bare")] == [1, 2, 0]
    assert struct.unpack_from("<QQQ", s["v2"], 8) == (BS, NB, N) and N - (NB - 1) * BS == 368
    return text, s


def readv(ctx, arena, stream, ranges, shift=0, cap=None, stream_at=IN_AT):
    """Runs one call into a GUARD-filled window; returns (out offsets, the bytes written) after
    checking that nothing outside [window, window + total) changed."""
    arena.fill()
    d_s = arena.put(stream, stream_at)
    offs = [r[0] for r in ranges]
    cnts = [r[1] for r in ranges]
    want_total = sum(min(c, N - o) if o < N else 0 for o, c in ranges)
    cap = want_total if cap is None else cap
    oo = ctx.readv_d2d(d_s, len(stream), offs, cnts, arena.base + OUT_AT + shift, cap)
    assert int(oo[0]) == 0 and int(oo[-1]) == want_total
    win = arena.get(OUT_AT - 64, want_total + shift + 64 + 4096)
    assert (win[:64 + shift] == GUARD).all(), "bytes before the output were written"
    assert (win[64 + shift + want_total:] == GUARD).all(), "bytes beyond h_out_offs[nranges] were written"
    return oo, win[64 + shift:64 + shift + want_total]


def expect(text, ranges) -> bytes:
    return b"".join(text[min(o, N):min(o, N) + min(c, N)].tobytes() for o, c in ranges)


SINGLE = [(0, 0), (0, 1), (4095, 2), (4096, 4096), (69_999, 1), (69_999, 10), (70_000, 5), (0, U64),
          (70_001, U64), (U64, U64), (4097, U64 - 4097), (65_536, 4096 + 368), (12_288, 0)]


@pytest.mark.parametrize("kind", ["v1", "v2", "bare"])
def test_single_ranges_equal_the_slice(ctx, arena, streams, kind):
    text, s = streams
    for r in SINGLE:
        oo, got = readv(ctx, arena, s[kind], [r])
        assert got.tobytes() == expect(text, [r]), (kind, r)
    assert len(expect(text, [(69_999, 10)])) == 1 and len(expect(text, [(70_000, 5)])) == 0
    assert expect(text, [(0, U64)]) == text.tobytes()
    # no ranges at all
    oo = ctx.readv_d2d(arena.put(s[kind], IN_AT), len(s[kind]), [], [], arena.base + OUT_AT, 0)
    assert oo.tolist() == [0]


def _alignment_ranges():
    """256 ranges of 33 bytes from sources k*257 + k%16, a range of k%16 bytes after each so the
    destinations move through every residue mod 16; then the piece lengths the kernel's head,
    body and tail turn on."""
    r = []
    for k in range(256):
        r.append((k * 257 + k % 16, 33))
        r.append((40_000 + 3 * k, k % 16))
    r += [(100, 0), (101, 1), (102, 15), (103, 16), (104, 17), (8197, 4097), (3, 4096), (4096, 4096), (69_632, 368)]
    return r


@pytest.mark.parametrize("kind", ["v1", "v2", "bare"])
def test_every_alignment_in_one_call(ctx, arena, streams, kind):
    text, s = streams
    ranges = _alignment_ranges()
    want = expect(text, ranges)
    dst = np.concatenate([[0], np.cumsum([c for _, c in ranges])])[:-1]
    big = [i for i, (_, c) in enumerate(ranges) if c == 33]
    assert {int(dst[i]) % 16 for i in big} == set(range(16))                       # every destination residue
    assert len({((ranges[i][0] - int(dst[i])) % 16) for i in big}) >= 8           # many relative alignments
    assert {0, 1, 15, 16, 17, 4097} <= {c for _, c in ranges}
    for shift in (0, 1, 3):
        oo, got = readv(ctx, arena, s[kind], ranges, shift=shift)
        assert [int(x) for x in oo[:-1]] == [int(x) for x in dst]
        assert got.tobytes() == want, (kind, shift)
    if kind == "bare":  # one block: every range is one piece, the 4097-byte one included
        ctx.set_timing(True)
        try:
            ctx.reset_stats()
            readv(ctx, arena, s[kind], ranges)
            assert ctx.kernel_stats()["gather_pieces"][0] == 2  # the record's header, then the pieces
        finally:
            ctx.set_timing(False)


def test_overlap_repeat_and_order_decode_each_block_once(ctx, arena, streams):
    text, s = streams
    many = [(5000, 9000)] * 3 + [(o, 700) for o in range(13_000, 5_000, -650)] + [(4096, 10_000), (13_999, 1)]
    one = [(4096, 10_000)]  # the same covering blocks: 1, 2 and 3
    assert {b for o, c in many for b in range(o // BS, (o + c - 1) // BS + 1)} == {1, 2, 3}
    ctx.set_timing(True)
    try:
        stats = []
        for ranges in (many, one):
            ctx.reset_stats()
            oo, got = readv(ctx, arena, s["v2"], ranges)
            assert got.tobytes() == expect(text, ranges)
            stats.append(ctx.kernel_stats())
    finally:
        ctx.set_timing(False)
    assert stats[0]["dec_lf_walk"][0] == stats[1]["dec_lf_walk"][0] == 1  # once per batch, not per range
    assert stats[0]["dec_headers"][0] == stats[1]["dec_headers"][0] == 1
    # the covered records' headers, then one launch for all the pieces of the batch
    assert stats[0]["gather_pieces"][0] == stats[1]["gather_pieces"][0] == 2


def test_scattered_blocks_are_decoded_in_one_batch(ctx, arena, streams):
    text, s = streams
    ranges = [(17 * BS + 5, 100), (2 * BS - 1, 2), (9 * BS, BS), (0, 1)]  # blocks 17, 1, 2, 9, 0
    ctx.set_timing(True)
    try:
        ctx.reset_stats()
        oo, got = readv(ctx, arena, s["v2"], ranges)
        st = ctx.kernel_stats()
    finally:
        ctx.set_timing(False)
    assert got.tobytes() == expect(text, ranges)
    assert st["dec_lf_walk"][0] == 1 and st["gather_pieces"][0] == 3  # headers, the records, the pieces


@pytest.mark.parametrize("kind", ["v1", "v2"])
def test_a_range_across_decode_batches(ctx, arena, streams, kind):
    text, s = streams
    ranges = [(4000, 30_000), (20_000, 5), (60_000, 9000), (3, 1)]
    try:
        ctx.set_option("max_batch", 8192)  # two blocks a batch
        ctx.set_timing(True)
        ctx.reset_stats()
        oo, got = readv(ctx, arena, s[kind], ranges)
        st = ctx.kernel_stats()
    finally:
        ctx.set_timing(False)
        ctx.set_option("max_batch", 0)
    assert got.tobytes() == expect(text, ranges)
    assert st["dec_lf_walk"][0] == 6  # blocks 0..8 and 14..16: twelve blocks, two a batch


def test_only_covering_blocks_are_read_and_checked(ctx, arena, streams):
    text, s = streams
    bad = flip_bit(s["v2"], crc_offset(s["v2"], 5) + 3, 7)
    ok = [(0, 5 * BS), (6 * BS, U64), (5 * BS - 1, 1), (6 * BS, 1)]
    oo, got = readv(ctx, arena, bad, ok)
    assert got.tobytes() == expect(text, ok)
    for ranges in ([(5 * BS, 1)], [(0, 1), (6 * BS - 1, 1)], [(0, U64)], [(5 * BS - 1, 2)]):
        with pytest.raises(bmh.BmhError) as e:
            readv(ctx, arena, bad, ranges)
        assert e.value.status == bmh.BMH_ECORRUPT and e.value.bad_block == 5, ranges
        assert "block 5" in str(e.value)
    with pytest.raises(bmh.BmhError) as e:
        ctx.verify_d2d(arena.put(bad, IN_AT), len(bad))
    assert e.value.status == bmh.BMH_ECORRUPT and e.value.bad_block == 5
    # the same flip in a version-1 container's place does not exist; a damaged record that no range
    # touches does not fail the call either: record 5's tree length zeroed
    o5 = 32 + 8 * NB + sum(struct.unpack_from("<Q", s["v1"], 32 + 8 * k)[0] for k in range(5))
    hurt = s["v1"][:o5 + 16] + bytes(8) + s["v1"][o5 + 24:]
    oo, got = readv(ctx, arena, hurt, ok)
    assert got.tobytes() == expect(text, ok)
    with pytest.raises(bmh.BmhError) as e:
        readv(ctx, arena, hurt, [(5 * BS, 1)])
    assert e.value.status == bmh.BMH_ECORRUPT and e.value.bad_block is None


def test_geometry_and_capacity(ctx, arena, streams):
    text, s = streams
    for kind in ("v1", "v2"):
        # block_size 4095 still gives ceil(70 000 / 4095) == 18 blocks, but no record holds 4095 bytes
        wrong = s[kind][:8] + struct.pack("<Q", BS - 1) + s[kind][16:]
        with pytest.raises(bmh.BmhError) as e:
            readv(ctx, arena, wrong, [(0, 1)])
        assert e.value.status == bmh.BMH_ECORRUPT and e.value.bad_block is None
        # ... and 2048 breaks the rule outright
        with pytest.raises(bmh.BmhError) as e:
            readv(ctx, arena, s[kind][:8] + struct.pack("<Q", 2048) + s[kind][16:], [(0, 1)])
        assert e.value.status == bmh.BMH_ECORRUPT
        # the whole-stream decode does not use the field: it answers as the host-buffer path does
        d_s = arena.put(wrong, IN_AT)
        want = raw_decompress_dev(ctx, np.frombuffer(wrong, np.uint8), cap=N)
        assert raw_decompress_d2d(ctx, d_s, len(wrong), arena.base + OUT_AT, cap=N) == want[:2]
        if want[0] == bmh.BMH_OK:
            assert arena.get(OUT_AT, want[1]).tobytes() == want[2]
    ranges = [(10, 100), (5000, 0), (69_990, 100), (4090, 12)]
    for cap in (121, 0):
        arena.fill()
        d_s = arena.put(s["v2"], IN_AT)
        with pytest.raises(bmh.BmhError) as e:
            ctx.readv_d2d(d_s, len(s["v2"]), [r[0] for r in ranges], [r[1] for r in ranges], arena.base + OUT_AT, cap)
        assert e.value.status == bmh.BMH_ERANGE and e.value.bad_block is None
        assert e.value.out_offs.tolist() == [0, 100, 100, 110, 122]  # filled all the same
        assert (arena.get(OUT_AT - 64, 4096) == GUARD).all()
    oo, got = readv(ctx, arena, s["v2"], ranges, cap=122)
    assert got.tobytes() == expect(text, ranges)
    # a stream placed at an odd address reads the same
    oo, got = readv(ctx, arena, s["v2"], ranges, stream_at=IN_AT + 1)
    assert got.tobytes() == expect(text, ranges)
