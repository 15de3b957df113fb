"""CPU: every hand-built record of tests/record_craft.py is a valid record by the reference's
definition, before the GPU decoder sees it (tests/test_gpu_decode_crafted.py): the oracle and
the host decoder restore its text and its MTF stream, and the reference's own DECOMPRESS
binary, where it has been built, reads the two longest-code records."""
import os
import subprocess

import numpy as np
import pytest

import bmh
import record_craft as rc
from oracle_ffi import REF_DIR


def test_tree_constructors():
    for side, codes in (("left", {0: "1", 1: "01", 2: "000", 3: "001"}), ("right", {0: "0", 1: "10", 2: "110", 3: "111"}),
                        ("alt", {0: "1", 1: "00", 2: "010", 3: "011"})):
        w = rc.code_words(rc.caterpillar([0, 1, 2, 3], side))
        assert {s: "".join(map(str, b)) for s, b in w.items()} == codes, side
    assert rc.tree_bytes(rc.caterpillar([7, 9], "left")) == bytes([0b10000001, 0b11000001, 0b00100000])
    assert rc.tree_bytes(5) == bytes([0b00000010, 0b10000000])
    w = rc.code_words(rc.complete(list(range(8))))
    assert all(len(w[s]) == 3 and int("".join(map(str, w[s])), 2) == s for s in range(8))
    t = rc.stride3(list(range(85)), 12, 5)
    w = rc.code_words(t)
    assert sorted(w) == list(range(85)) and rc.max_code_len(t) == 36
    assert all(len(w[s]) == 3 * (min(s // 7, 11) + 1) for s in range(85))
    assert all("".join(map(str, w[s][3 * lv:3 * lv + 3])) == "101" for s in range(85) for lv in range(min(s // 7, 11)))
    for d in (12, 64, 65, 100):
        assert rc.max_code_len(rc.caterpillar(range(d + 1), "alt")) == d


def test_case_shapes():
    """The shapes the GPU tests rely on: code lengths, segment counts, header edges."""
    def pay_bits(c):
        return 8 * (len(c.rec) - rc.payload_offset(c.rec))
    for d in rc.LONG_DEPTHS:
        c = rc.get(f"cat{d}_right")
        assert len(c.text) == rc.LONG_N and 17 <= -(-pay_bits(c) // 8192) <= 85, d
        # anti-Huffman: the two commonest MTF values carry the two longest codes
        w = rc.code_words(c.tree)
        assert [len(w[s]) for s in rc.rarest_first(c.mtf, d + 1)[-2:]] == [d, d]
    c = rc.get("stride3")
    assert -(-pay_bits(c) // 8192) == 50  # ~20.3 bits a symbol
    c = rc.get("complete256_8192")
    assert int.from_bytes(c.rec[16:24], "little") == 320 and pay_bits(c) == 65536
    for n in (24576, 24577, 8191):
        assert pay_bits(rc.get(f"two_leaf_{n}")) == (n + 7) // 8 * 8
    assert len(rc.get("single_4097").rec) == 24 + 2 + 1
    assert len(set(rc.get("unused_leaves").mtf)) == 5
    for n in rc.LF_SIZES:
        for p in rc.lf_primaries(n):
            c = rc.get(f"lf_n{n}_p{p}")
            assert len(c.text) == n and int.from_bytes(c.rec[:8], "little") == p
    for ulen, k, ranks in rc.PERIODIC:
        for r in ranks:
            c = rc.get(f"per_u{ulen}_k{k}_r{r}")
            assert len(c.text) == ulen * k and c.text == c.text[:ulen] * k
            assert int.from_bytes(c.rec[:8], "little") == k * r
    # the big block: n a multiple of 256, and along the LF cycle some stretch between two
    # splitter rows (rows 0 mod 256 and the primary) is longer than the decoder's 1024-byte slot
    c = rc.get(rc.LF_BIG_CASE)
    n, primary = len(c.text), int.from_bytes(c.rec[:8], "little")
    assert n % 256 == 0
    L = np.frombuffer(rc.oracle().bwt(c.text)[1], np.uint8)
    nxt = np.argsort(L, kind="stable").tolist()  # row -> the row of the next text position
    row, run, longest = primary, 0, 0
    for _ in range(n):
        row = nxt[row]
        run += 1
        if row % 256 == 0 or row == primary:
            longest, run = max(longest, run), 0
    assert row == primary and longest > 1024


@pytest.mark.parametrize("name", rc.ALL_CASES)
def test_oracle_and_host_decode(oracle, name):
    c = rc.get(name)
    assert oracle.decode(c.rec) == c.text
    assert bmh.decompress_bytes(c.rec) == c.text
    assert oracle.decode_to_mtf(c.rec) == c.mtf
    assert bmh.record_to_mtf(c.rec) == c.mtf


def test_unaligned_batch_covers_every_residue():
    batch = rc.unaligned_batch()
    r16, o16, p4 = rc.batch_residues(batch)
    assert r16 == set(range(16)) and o16 == set(range(16)) and p4 == set(range(4))
    names = {c.name for c in batch}
    assert set(rc.LONG_CASES + rc.NOSYNC_CASES + rc.EDGE_CASES + rc.LF_CASES + rc.PERIODIC_CASES) <= names
    assert rc.LF_BIG_CASE in names and any(len(c.text) <= 3 for c in batch)


@pytest.mark.parametrize("name", ["cat64_right", "stride3"])
def test_reference_binary_decodes(oracle, tmp_path, name):
    """The reference's own decompress(), where oracle/_ref has been built, on the depth-64
    caterpillar and the stride-3 record (the oracle stands in for it elsewhere)."""
    c = rc.get(name)
    assert rc.max_code_len(c.tree) == {"cat64_right": 64, "stride3": 36}[name]
    assert oracle.decode(c.rec) == c.text
    dec = os.path.join(REF_DIR, "ref_DECOMPRESS")
    if os.path.exists(dec):
        (tmp_path / "in.bzap").write_bytes(c.rec)
        subprocess.run([dec, "in.bzap", "out.ref"], cwd=tmp_path, check=True, capture_output=True, timeout=120)
        assert (tmp_path / "out.ref").read_bytes() == c.text
