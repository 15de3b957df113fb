"""GPU decoder (csrc/decode.hip) on records it did not write: hand-built prefix-code trees with
codes of up to 64 bits, primary rows and block lengths placed on the LF splitter edges,
periodic texts, segment / header edges and one batch at every alignment. The records come
from tests/record_craft.py; tests/test_record_craft.py has already shown that the oracle and
the host decoder restore each of them, so the reference here is the plain text a record was
built from, compared bit-exact. No record here is malformed except the depth-65 one, which the
host side of the decoder refuses before any kernel is launched."""
import numpy as np
import pytest

import bmh
import record_craft as rc
from bmh import synth

pytestmark = pytest.mark.gpu


def _decode_batch(ctx, recs):
    """One decode_blocks_dev call over the records laid back to back; returns the blocks."""
    ro = np.zeros(len(recs) + 1, np.uint64)
    ro[1:] = np.cumsum([len(r) for r in recs])
    ns = [int.from_bytes(r[8:16], "little") for r in recs]
    total = sum(ns)
    d_rec, d_out = ctx.alloc(int(ro[-1])), ctx.alloc(total)
    try:
        d_rec.upload(np.frombuffer(b"".join(recs), np.uint8))
        oo = ctx.decode_blocks_dev(d_rec, ro, d_out, total)
        assert oo.tolist() == np.concatenate([[0], np.cumsum(ns)]).tolist()
        raw = d_out.download(total).tobytes()
    finally:
        d_rec.free()
        d_out.free()
    return [raw[int(oo[i]):int(oo[i + 1])] for i in range(len(recs))]


def _first_diff(a: bytes, b: bytes) -> str:
    if len(a) != len(b):
        return f"length {len(a)} != {len(b)}"
    x, y = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    bad = np.flatnonzero(x != y)
    return "equal" if bad.size == 0 else f"{bad.size} of {len(a)} bytes differ, first at {int(bad[0])}"


@pytest.fixture(scope="module")
def zipf_rec(ctx):
    text = synth.zipf_text(50_000).tobytes()
    return rc.Case("zipf_50000", text, ctx.encode_blocks([text])[0], b"")


# ---- 1. long codes: 12 / 13 straddle the LUT width, 32 / 33 the bit window's guarantee, 64 is
# the admitted maximum; 17-85 segments each, so pass 1, the fix-up rounds and pass 3 all run
@pytest.mark.parametrize("side", rc.SIDES)
@pytest.mark.parametrize("d", rc.LONG_DEPTHS)
def test_long_codes(ctx, d, side):
    c = rc.get(f"cat{d}_{side}")
    got = ctx.decompress_bytes(c.rec)
    assert got == c.text, _first_diff(got, c.text)


# ---- 2. the limit: 65-bit codes are refused on the host, before any kernel
def test_code_length_limit(ctx):
    c = rc.get(rc.LIMIT_CASE)
    assert rc.max_code_len(c.tree) == 65
    ctx.reset_stats()
    ctx.set_timing(True)
    try:
        with pytest.raises(bmh.BmhError) as e:
            ctx.decompress_bytes(c.rec)
        assert e.value.status == bmh.BMH_ECORRUPT, e.value
        assert not [k for k in ctx.kernel_stats() if k.startswith("dec_") and k != "dec_headers"]
    finally:
        ctx.set_timing(False)
    good = rc.get("cat64_alt")
    assert ctx.decompress_bytes(good.rec) == good.text
    assert bmh.decompress_bytes(c.rec) == c.text  # the host decoder has no such limit


# ---- 3. long codes that never resynchronise (every length a multiple of 3, 8192 is not)
def test_stride3_offset_map(ctx, zipf_rec):
    c = rc.get("stride3")
    ctx.reset_stats()
    ctx.set_timing(True)
    try:
        got = ctx.decompress_bytes(c.rec)
        assert got == c.text, _first_diff(got, c.text)
        assert "dec_huff_map" in ctx.kernel_stats()  # the fix-up rounds cannot settle this
    finally:
        ctx.set_timing(False)
    batch = [c, rc.get("complete8_100k"), zipf_rec]
    for b, got in zip(batch, _decode_batch(ctx, [b.rec for b in batch])):
        assert got == b.text, (b.name, _first_diff(got, b.text))


# ---- 4. segment and header edges
@pytest.mark.parametrize("name", rc.EDGE_CASES)
def test_segment_and_header_edges(ctx, name):
    c = rc.get(name)
    got = ctx.decompress_bytes(c.rec)
    assert got == c.text, _first_diff(got, c.text)


@pytest.mark.parametrize("name", ["single_1", "single_4097"])
def test_single_leaf_between_records(ctx, name):
    batch = [rc.get("cat13_left"), rc.get(name), rc.get("unused_leaves")]
    for b, got in zip(batch, _decode_batch(ctx, [b.rec for b in batch])):
        assert got == b.text, (b.name, _first_diff(got, b.text))


# ---- 5. one batch with record, payload and output offsets on every residue
def test_unaligned_batch(ctx, zipf_rec):
    batch = rc.unaligned_batch() + [zipf_rec, rc.get("filler3_1"), rc.get("cat33_alt")]
    r16, o16, p4 = rc.batch_residues(batch)
    assert len(r16) == 16 and len(o16) == 16 and len(p4) == 4
    got = _decode_batch(ctx, [b.rec for b in batch])
    bad = [(b.name, _first_diff(g, b.text)) for b, g in zip(batch, got) if g != b.text]
    assert not bad, bad
    alone = {}
    for b, g in zip(batch, got):
        if b.name not in alone:
            alone[b.name] = ctx.decompress_bytes(b.rec)
        assert g == alone[b.name], b.name


# ---- 6. primary row and length on the splitter edges (rows 0 mod 256 and the primary)
@pytest.mark.parametrize("n", rc.LF_SIZES)
def test_primary_on_splitter_edges(ctx, n):
    for p in rc.lf_primaries(n):
        c = rc.get(f"lf_n{n}_p{p}")
        got = ctx.decompress_bytes(c.rec)
        assert got == c.text, (p, _first_diff(got, c.text))


def test_length_multiple_of_256_long_segments(ctx):
    c = rc.get(rc.LF_BIG_CASE)
    got = ctx.decompress_bytes(c.rec)
    assert got == c.text, _first_diff(got, c.text)


# ---- 7. periodic text u^k: k LF cycles, the primary on k * rank(u)
@pytest.mark.parametrize("ulen,k,ranks", rc.PERIODIC)
def test_periodic_text(ctx, ulen, k, ranks):
    for r in ranks:
        c = rc.get(f"per_u{ulen}_k{k}_r{r}")
        got = ctx.decompress_bytes(c.rec)
        assert got == c.text, (r, _first_diff(got, c.text))


# ---- 8. the u32 / u64 LF entry switch at 2^24 rows
def test_lf_entry_width_switch(ctx):
    sizes = [1 << 24, 5000, (1 << 24) + 1, 257]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    total = int(offs[-1])
    cap = sum(int(bmh.lib().bmh_record_bound(s)) for s in sizes)
    d_in, d_rec, d_dec = ctx.alloc(total), ctx.alloc(cap), ctx.alloc(total)
    try:
        ctx.synth_splitmix64(d_in, total, 24, 0)
        ro = ctx.encode_blocks_dev(d_in, offs, d_rec, cap)
        want = d_in.download().tobytes()
        oo = ctx.decode_blocks_dev(d_rec, ro, d_dec, total)  # one block > 2^24: u64 entries
        assert (oo == offs).all()
        assert d_dec.download().tobytes() == want
        d_dec.upload(np.zeros(total, np.uint8))
        oo = ctx.decode_blocks_dev(d_rec, ro[:3], d_dec, total)  # u32 entries at exactly 2^24
        assert (oo == offs[:3]).all()
        assert d_dec.download(int(offs[2])).tobytes() == want[:int(offs[2])]
    finally:
        d_in.free()
        d_rec.free()
        d_dec.free()
