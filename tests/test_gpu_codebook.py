"""k_huff_build, k_rec_offs and k_rec_headers (csrc/huffman.hip) driven through
Context.codebook_dev with the crafted histograms of tests/huff_families.py: frequency groups of
internal nodes wider than a 64-node word, indices on a word's last bit, pure heap-order chains,
the u32 top of the frequency range, and the heap-history order of blocks below 128 KiB.
tests/test_huff_families.py has shown on the CPU that the references used here (the oracle's tree
for blocks from 2^17 bytes, a plain priority queue over the glibc restatement's ranks below) agree
with the host build and the rounds restatement on every case. Compared bit-exact: code, len, tree,
tree_len and leaves of every table, every record's extent, every header in place, and the
sentinel fill of every byte that is no header."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import bmh
import huff_families as hf
from bmh import synth
from oracle_ffi import GOLDEN

pytestmark = pytest.mark.gpu

TABLE = np.dtype([("code", "<u8", 256), ("len", "u1", 256), ("tree", "u1", 320), ("tree_len", "<u4"),
                  ("leaves", "<u4")])
SENTINEL = 0xA5
_REFS: dict = {}


def _ref(case: hf.Case, oracle):
    """The expected table of a case as one TABLE row, and its payload size; computed once."""
    r = _REFS.get(case.name)
    if r is None:
        ln, code, tree = hf.reference_tables(case, oracle)
        row = np.zeros((), TABLE)
        row["code"], row["len"] = np.array(code, np.uint64), np.array(ln, np.uint8)
        row["tree"][:len(tree)] = np.frombuffer(tree, np.uint8)
        row["tree_len"], row["leaves"] = len(tree), case.leaves
        r = _REFS[case.name] = (row, hf.payload_bytes(case.freq, ln))
    return r


def _run(ctx, oracle, cases, with_out=True, seed=0):
    """One codebook_dev call over `cases` and the comparison of everything it returns."""
    assert bmh.CodeTable.code.offset == 0 and TABLE.itemsize == ctypes.sizeof(bmh.CodeTable)
    rng = np.random.default_rng(seed)
    nb = len(cases)
    freq = np.stack([c.freq for c in cases])
    first = np.stack([c.first for c in cases])
    prim = np.array([int(rng.integers(0, c.n)) for c in cases], np.uint64)
    offs = np.concatenate([[0], np.cumsum([c.n for c in cases], dtype=np.uint64)]).astype(np.uint64)
    want = np.stack([_ref(c, oracle)[0] for c in cases])
    ext = np.array([24 + int(w["tree_len"]) + _ref(c, oracle)[1] for c, w in zip(cases, want)], np.uint64)
    want_ro = np.concatenate([[0], np.cumsum(ext, dtype=np.uint64)]).astype(np.uint64)
    cap = int(want_ro[-1]) + 64
    d_out = ctx.alloc(cap) if with_out else None
    try:
        if with_out:
            d_out.upload(np.full(cap, SENTINEL, np.uint8))
        tabs, ro = ctx.codebook_dev(freq, first, prim, offs, d_out, cap if with_out else 0)
        raw = d_out.download() if with_out else None
    finally:
        if with_out:
            d_out.free()
    got = np.frombuffer(tabs, TABLE, nb)
    for field in TABLE.names:
        bad = [cases[b].name for b in range(nb) if not np.array_equal(got[field][b], want[field][b])]
        assert not bad, (field, len(bad), bad[:5])
    assert np.array_equal(ro, want_ro), [cases[b].name for b in np.flatnonzero(np.diff(ro) != ext)[:5]]
    if with_out:
        exp = np.full(cap, SENTINEL, np.uint8)
        for b, (c, w) in enumerate(zip(cases, want)):
            tl = int(w["tree_len"])
            hdr = b"".join(int(v).to_bytes(8, "little") for v in (prim[b], c.n, tl)) + w["tree"][:tl].tobytes()
            exp[int(ro[b]):int(ro[b]) + len(hdr)] = np.frombuffer(hdr, np.uint8)
        diff = np.flatnonzero(raw != exp)
        assert diff.size == 0, (diff.size, int(diff[0]), int(np.searchsorted(ro, diff[0], "right")) - 1)
    return got, ro


# ---- 1. the closed-form (model) path
def test_model_path_one_batch(ctx, oracle):
    cases = list(hf.model_cases())
    assert 100 <= len(cases) <= 256  # k_rec_offs copies the headers itself
    _run(ctx, oracle, cases)


def test_model_path_more_than_1024_blocks(ctx, oracle):
    """The same set ten times over, shuffled: k_rec_headers copies the headers, k_rec_offs scans
    in two 1024-wide steps with a carry; every block equals its expected table wherever it lies."""
    cases = list(hf.model_cases()) * 10
    assert len(cases) > 1024
    order = np.random.default_rng(3).permutation(len(cases))
    _run(ctx, oracle, [cases[i] for i in order], seed=3)


def test_fibonacci_chains_without_output(ctx, oracle):
    """Reversed Fibonacci(40) and Fibonacci(45) in every variant: hundreds of MiB to GiB per
    block, so tables and offsets only; batched as far as the 4 GiB batch limit allows."""
    group, total = [], 0
    for c in hf.big_model_cases() + (None,):
        if c is None or total + c.n >= 0xFFFFFFFF:
            _run(ctx, oracle, group, with_out=False)
            group, total = [], 0
        if c is not None:
            group.append(c)
            total += c.n


# ---- 2. the heap-history path
def test_heap_history_mixed_with_model_blocks(ctx, oracle):
    """Every heap-history case in one batch between model-path blocks (a block must not pick up
    a neighbour's rank table; several blocks of one size carry different histograms), once in a
    batch k_rec_offs finishes itself and once shuffled in a batch of more than 256 blocks."""
    hist, model = list(hf.history_cases()), [c for c in hf.model_cases() if c.n < 1 << 18]
    mixed = []
    for i, c in enumerate(hist):
        mixed.append(c)
        if i % 3 == 0:
            mixed.append(model[(7 * i) % len(model)])
    assert len(hist) >= 40 and len(mixed) <= 256
    _run(ctx, oracle, mixed, seed=1)
    big = mixed * 3
    assert len(big) > 256
    order = np.random.default_rng(5).permutation(len(big))
    _run(ctx, oracle, [big[i] for i in order], seed=2)


# ---- 3. the top of the frequency range
@pytest.mark.parametrize("i", [0, 1])
def test_top_of_range(ctx, oracle, i):
    c = hf.top_cases()[i]
    got, ro = _run(ctx, oracle, [c], with_out=False)
    if i == 0:  # two one-bit codes over 2^32 - 2 symbols
        assert int(ro[1]) == 24 + 3 + (2**32 - 2) // 8 + 1
    else:
        assert int(got["len"][0].max()) == 44


# ---- 4. the kernel alone against the whole encode
def test_headers_equal_the_encodes(ctx, oracle):
    blocks = [synth.zipf_text(200_000).tobytes(), synth.splitmix64_bytes(0, 0, 200_000).tobytes()]
    recs = ctx.encode_blocks(blocks)
    freq, first, prim = [], [], []
    for data in blocks:
        p, L = oracle.bwt(data)
        f, fi = oracle.histogram(oracle.mtf(L))
        freq.append(f)
        first.append(fi)
        prim.append(p)
    offs = np.array([0, 200_000, 400_000], np.uint64)
    cap = sum(len(r) for r in recs)
    d_out = ctx.alloc(cap)
    try:
        d_out.upload(np.full(cap, SENTINEL, np.uint8))
        tabs, ro = ctx.codebook_dev(np.stack(freq), np.stack(first), prim, offs, d_out, cap)
        raw = d_out.download()
    finally:
        d_out.free()
    assert ro.tolist() == [0, len(recs[0]), len(recs[0]) + len(recs[1])]
    for b, rec in enumerate(recs):
        h = 24 + tabs[b].tree_len
        assert raw[int(ro[b]):int(ro[b]) + h].tobytes() == rec[:h], b
        assert (raw[int(ro[b]) + h:int(ro[b + 1])] == SENTINEL).all(), b
        assert rec == oracle.encode(blocks[b]), b


# ---- 5. the context's cached workspace tags
def _band_sha(kind: str, n: int) -> str:
    man = json.load(open(os.path.join(GOLDEN, "manifests", "bands.json")))
    return next(e["sha256"] for e in man["cases"] if e["kind"] == kind and e["n"] == n)


def _crafted(sizes, tag):
    """One crafted histogram per block size, differing from what the block's own bytes give."""
    return [hf.make_case(f"{tag}_{n}", "history" if n < hf.BAND_CEIL else "model",
                         hf.staircase_topped(n, 256) if i % 2 else hf.near_equal(n, 255), n, 1 + i % 2)
            for i, n in enumerate(sizes)]


def _check_records(recs, blocks, oracle):
    for rec, data in zip(recs, blocks):
        if len(data) < hf.BAND_CEIL:  # a band size: the reference's own record (bands.json)
            assert hashlib.sha256(rec).hexdigest() == _band_sha("zipf", len(data)), len(data)
        else:
            assert rec == oracle.encode(data), len(data)


def test_context_hygiene(ctx, oracle):
    """encode, codebook_dev with the same block sizes and other histograms, encode again: the
    records are unchanged and the reference's. Three blocks run on one pipeline, so all three
    calls share the context's own workspaces (status word, block offsets, band tables,
    freq / first / primary). Then the other order on a layout the context has not seen."""
    z = synth.zipf_text(70_000).tobytes()
    blocks = [z[:42000], synth.splitmix64_bytes(0, 0, 150_000).tobytes(), z[:4250]]
    r1 = ctx.encode_blocks(blocks)
    assert ctx.last_pipelines() == 1
    _check_records(r1, blocks, oracle)
    crafted = _crafted([len(b) for b in blocks], "hygiene_a")
    _run(ctx, oracle, crafted, seed=11)
    r2 = ctx.encode_blocks(blocks)
    assert ctx.last_pipelines() == 1 and r2 == r1
    _run(ctx, oracle, crafted, with_out=False, seed=12)
    assert ctx.encode_blocks(blocks) == r1
    # codebook_dev first
    blocks = [z[:10000], synth.splitmix64_bytes(5, 0, 140_000).tobytes(), z[:63800]]
    crafted = _crafted([len(b) for b in blocks], "hygiene_b")
    g1, ro1 = _run(ctx, oracle, crafted, seed=13)
    recs = ctx.encode_blocks(blocks)
    assert ctx.last_pipelines() == 1
    _check_records(recs, blocks, oracle)
    g2, ro2 = _run(ctx, oracle, crafted, seed=13)
    assert g1.tobytes() == g2.tobytes() and np.array_equal(ro1, ro2)


# ---- 6. validation on the host
def test_validation(ctx, oracle):
    good = [hf.history_cases()[5], hf.model_cases()[40], hf.history_cases()[-1]]
    sizes = [c.n for c in good]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    freq, first = np.stack([c.freq for c in good]), np.stack([c.first for c in good])
    prim = np.array([0, sizes[1] - 1, 3], np.uint64)

    def call(f=freq, fi=first, p=prim, d_out=None, cap=0):
        return ctx.codebook_dev(f, fi, p, offs, d_out, cap)

    def present(b):
        return [int(s) for s in np.flatnonzero(freq[b])]

    bad = []
    f = freq.copy()
    f[1, present(1)[0]] += 1
    bad.append(("sum above the size", dict(f=f)))
    f = freq.copy()
    f[2, present(2)[1]] -= 1
    bad.append(("sum below the size", dict(f=f)))
    f = freq.copy()
    f[0, present(0)[0]] = 2**64 - 1  # a sum that wraps
    bad.append(("sum wraps", dict(f=f)))
    fi = first.copy()
    a, b_ = present(1)[:2]
    fi[1, a] = fi[1, b_]
    bad.append(("duplicate first", dict(fi=fi)))
    fi = first.copy()
    fi[2, present(2)[0]] = sizes[2]
    bad.append(("first >= n", dict(fi=fi)))
    p = prim.copy()
    p[1] = sizes[1]
    bad.append(("primary >= n", dict(p=p)))
    f = freq.copy()
    f[0] = 0
    bad.append(("empty histogram", dict(f=f)))
    ctx.reset_stats()
    ctx.set_timing(True)
    try:
        for what, kw in bad:
            with pytest.raises(bmh.BmhError) as e:
                call(**kw)
            assert e.value.status == bmh.BMH_EINVAL, (what, e.value)
        assert "huff_build" not in ctx.kernel_stats()  # refused before any launch
    finally:
        ctx.set_timing(False)
    # a first position where the frequency is 0 is ignored
    fi = first.copy()
    fi[0, np.flatnonzero(freq[0] == 0)] = 0
    t_ign, ro_ign = call(fi=fi)
    t_ok, ro_ok = _run(ctx, oracle, good, with_out=False)
    assert np.frombuffer(t_ign, TABLE, 3).tobytes() == t_ok.tobytes() and np.array_equal(ro_ign, ro_ok)
    # a capacity one byte short: BMH_ERANGE and nothing written; then the exact capacity
    total = int(ro_ok[-1])
    d_out = ctx.alloc(total)
    try:
        d_out.upload(np.full(total, SENTINEL, np.uint8))
        with pytest.raises(bmh.BmhError) as e:
            call(d_out=d_out, cap=total - 1)
        assert e.value.status == bmh.BMH_ERANGE, e.value
        assert (d_out.download() == SENTINEL).all()
        t2, ro2 = call(d_out=d_out, cap=total)
        assert np.array_equal(ro2, ro_ok) and np.frombuffer(t2, TABLE, 3).tobytes() == t_ok.tobytes()
        raw = d_out.download()
        for b in range(3):
            assert int.from_bytes(raw[int(ro2[b]) + 8:int(ro2[b]) + 16].tobytes(), "little") == sizes[b]
    finally:
        d_out.free()
    with pytest.raises(bmh.BmhError) as e:
        ctx.codebook_dev(freq[:0], first[:0], prim[:0], offs[:1])
    assert e.value.status == bmh.BMH_EINVAL
