"""Hand-built records for the decoders: a text, an arbitrary prefix-code tree, a chosen primary.

A record is `u64 primary | u64 n | u64 tree_len | tree | payload` (compress(), main.cpp:300-325).
The tree is written in preorder, one bit 1 for an inner node followed by its left and right
subtrees, or 0 and 8 symbol bits for a leaf (dfs, main.cpp:174-187), zero-padded to whole
bytes; the payload is the code words of the MTF stream MSB-first, zero-padded, at least one
byte (encode_with_huffman, main.cpp:158-172). decompress() reads any prefix code, so a record
need not carry the tree huffman() would have built: the trees here are caterpillars (one leaf
per depth), complete trees and a 3-bit-per-level chain, with the block's commonest MTF values
on the LONGEST codes, so codes of up to 64 bits (and beyond) are frequent in 20 000 symbols.

Trees are nested pairs `(left, right)` with integer leaves. Everything is generated from fixed
seeds; CASES maps each case name to its builder and `get(name)` caches the built case, so the
CPU tests (tests/test_record_craft.py: oracle and host decoder accept every record) and the
GPU tests (tests/test_gpu_decode_crafted.py) share one list.
"""
from __future__ import annotations

import functools
import sys
from typing import Callable, NamedTuple

import numpy as np

from oracle_ffi import Oracle

SIDES = ("left", "right", "alt")
LONG_DEPTHS = (12, 13, 31, 32, 33, 40, 44, 45, 63, 64)
LONG_N = 20_000


class Case(NamedTuple):
    name: str
    text: bytes
    rec: bytes
    mtf: bytes  # the MTF stream the payload encodes
    tree: object = None  # the hand-built tree (None: the record is the reference encoder's)


@functools.lru_cache(maxsize=None)
def oracle() -> Oracle:
    return Oracle()


# ------------------------------------------------------------------------------ trees
def caterpillar(symbols, side: str):
    """Leaves at depths 1, 2, ..., d, d for d + 1 symbols, symbols[0] the shallowest. `side`
    is where the spine goes: "left" (the long codes are 0-bits), "right" (1-bits) or "alt"
    (left at even depths, right at odd ones)."""
    symbols = list(symbols)
    if len(symbols) < 2:
        raise ValueError("a caterpillar needs two leaves")
    d = len(symbols) - 1
    t = (symbols[d - 1], symbols[d])
    for i in range(d - 2, -1, -1):
        left = side == "left" or (side == "alt" and i % 2 == 0)
        t = (t, symbols[i]) if left else (symbols[i], t)
    return t


def complete(symbols):
    """Every code the same length: leaves left to right in the order given (a power of two)."""
    symbols = list(symbols)
    if len(symbols) & (len(symbols) - 1) or not symbols:
        raise ValueError("a complete tree needs a power of two of leaves")
    if len(symbols) == 1:
        return symbols[0]
    h = len(symbols) // 2
    return (complete(symbols[:h]), complete(symbols[h:]))


def stride3(symbols, levels: int, cont_slot: int):
    """A chain of 3-bit levels: each has 7 leaves and, in slot cont_slot, the next level; the
    last level has 8 leaves. 7 * (levels - 1) + 8 symbols, symbols[0:7] the shallowest; every
    code length is a multiple of 3, up to 3 * levels."""
    symbols = list(symbols)
    if len(symbols) != 7 * (levels - 1) + 8:
        raise ValueError("stride3: 7 * (levels - 1) + 8 symbols")
    t = complete(symbols[7 * (levels - 1):])
    for lv in range(levels - 2, -1, -1):
        slots = symbols[7 * lv:7 * lv + 7]
        slots.insert(cont_slot, None)
        sub = complete(slots)
        t = _replace_none(sub, t)
    return t


def _replace_none(tree, sub):
    if tree is None:
        return sub
    if isinstance(tree, tuple):
        return (_replace_none(tree[0], sub), _replace_none(tree[1], sub))
    return tree


def tree_bytes(tree) -> bytes:
    bits: list[int] = []

    def dfs(t):
        if isinstance(t, tuple):
            bits.append(1)
            dfs(t[0])
            dfs(t[1])
        else:
            bits.append(0)
            bits.extend((int(t) >> b) & 1 for b in range(7, -1, -1))
    dfs(tree)
    return np.packbits(np.array(bits, np.uint8)).tobytes()


def code_words(tree) -> dict[int, np.ndarray]:
    """symbol -> its code word as an array of bits (left = 0, right = 1; a lone leaf: empty)."""
    out: dict[int, np.ndarray] = {}

    def dfs(t, path):
        if isinstance(t, tuple):
            dfs(t[0], path + [0])
            dfs(t[1], path + [1])
        else:
            if int(t) in out:
                raise ValueError("symbol twice in the tree")
            out[int(t)] = np.array(path, np.uint8)
    dfs(tree, [])
    return out


def max_code_len(tree) -> int:
    return max(len(w) for w in code_words(tree).values())


def pack(m: bytes, tree) -> bytes:
    words = code_words(tree)
    a = np.frombuffer(m, np.uint8)
    bits = np.concatenate([words[int(v)] for v in a]) if a.size else np.zeros(0, np.uint8)
    out = np.packbits(bits).tobytes()
    return out if out else b"\x00"


def record(primary: int, n: int, tree, m: bytes) -> bytes:
    tb = tree_bytes(tree)
    return np.array([primary, n, len(tb)], np.uint64).tobytes() + tb + pack(m, tree)


def rarest_first(m: bytes, k: int) -> list[int]:
    """MTF values 0 .. k-1 by their count in m, rarest first (ties: the smaller value): the
    constructors put the first ones on the short codes, an anti-Huffman assignment."""
    freq = np.bincount(np.frombuffer(m, np.uint8), minlength=k)
    if freq.size > k:
        raise ValueError("MTF value outside the alphabet")
    return sorted(range(k), key=lambda s: (int(freq[s]), s))


def craft(name: str, text: bytes, make_tree: Callable[[list[int]], object], k: int) -> Case:
    """The record of `text` (byte values below k) under the tree make_tree(rarest-first MTF
    values) instead of huffman()'s."""
    primary, L = oracle().bwt(text)
    m = oracle().mtf(L)
    tree = make_tree(rarest_first(m, k))
    return Case(name, text, record(primary, len(text), tree, m), m, tree)


def encoded(name: str, text: bytes) -> Case:
    """The reference's own record of `text` (oracle.encode)."""
    m = oracle().mtf(oracle().bwt(text)[1])
    return Case(name, text, oracle().encode(text), m)


def random_text(seed: int, n: int, k: int) -> bytes:
    return np.random.default_rng(seed).integers(0, k, n, dtype=np.uint8).tobytes()


# ------------------------------------------------------------------- primary control
def rotation_starts(t: bytes) -> list[int]:
    """Start positions of the rotations of t in sorted order; raises if two rotations are equal
    (t periodic)."""
    n = len(t)
    tt = t + t
    sa = sorted(range(n), key=lambda i: tt[i:i + n])
    for a, b in zip(sa, sa[1:]):
        if tt[a:a + n] == tt[b:b + n]:
            raise ValueError("periodic text")
    return sa


def aperiodic_text(seed: int, n: int, k: int) -> tuple[bytes, list[int]]:
    """Random text over k byte values whose n rotations are all different, with their sorted
    starts (the seed is advanced past periodic draws, which only tiny n can give)."""
    for s in range(seed, seed + 64):
        t = random_text(s, n, k)
        try:
            return t, rotation_starts(t)
        except ValueError:
            continue
    raise AssertionError("no aperiodic text found")


def with_primary(t: bytes, sa: list[int], r: int) -> bytes:
    """The rotation of the aperiodic text t whose BWT has primary row r."""
    return t[sa[r]:] + t[:sa[r]]


def lf_primaries(n: int) -> list[int]:
    return sorted({p for p in (0, 1, 255, 256, 257, n - 1, 256 * ((n - 1) // 256)) if 0 <= p < n})


LF_SIZES = (1, 2, 255, 256, 257, 512, 4095, 4096, 4097)
LF_BIG_N = 300_032  # a multiple of 256, ~1173 splitters
PERIODIC = ((256, 2, (0, 128, 255)), (255, 3, (0, 127, 254)), (1, 300, (0,)), (2, 128, (0, 1)),
            (257, 256, (0, 128, 256)), (1000, 5, (0, 500, 999)))


def _lf_case(n: int, p: int) -> Case:
    t, sa = aperiodic_text(1000 + n, n, 4)
    text = with_primary(t, sa, p)
    c = encoded(f"lf_n{n}_p{p}", text)
    assert int.from_bytes(c.rec[:8], "little") == p, "primary control"
    return c


def _periodic_case(ulen: int, k: int, rank: int) -> Case:
    """u^k, u rotated to rank `rank` among its rotations: the primary row is k * rank."""
    u, sa = aperiodic_text(2000 + ulen, ulen, 4) if ulen > 2 else ((b"\x03", [0]) if ulen == 1 else (b"\x01\x02", [0, 1]))
    text = with_primary(u, sa, rank) * k
    c = encoded(f"per_u{ulen}_k{k}_r{rank}", text)
    assert int.from_bytes(c.rec[:8], "little") == k * rank, "primary control (periodic)"
    return c


# ------------------------------------------------------------------------- the cases
def _long(d: int, side: str) -> Case:
    text = random_text(100 * d + SIDES.index(side), LONG_N, d + 1)
    return craft(f"cat{d}_{side}", text, lambda s: caterpillar(s, side), d + 1)


def _stride3() -> Case:
    return craft("stride3", random_text(3, LONG_N, 85), lambda s: stride3(s, 12, 5), 85)


def _complete8() -> Case:
    return craft("complete8_100k", random_text(8, 100_000, 8), complete, 8)


def _complete256() -> Case:
    perm = np.random.default_rng(256).permutation(256).tolist()
    return craft("complete256_8192", random_text(257, 8192, 256), lambda s: complete(perm), 256)


def _two_leaf(n: int) -> Case:
    return craft(f"two_leaf_{n}", random_text(n, n, 2), lambda s: (s[0], s[1]), 2)


def _single(n: int) -> Case:
    return craft(f"single_{n}", bytes(n), lambda s: s[0], 1)


def _unused_leaves() -> Case:
    # the text has 5 byte values; the tree has leaves for 16, eleven of which never occur
    return craft("unused_leaves", random_text(5, 5000, 5), lambda s: complete(list(range(5, 16)) + s), 5)


def _filler(n: int, v: int) -> Case:
    """A 1-, 2- or 3-byte block (the unaligned batch puts these between the others)."""
    text = bytes((v + i) % 3 for i in range(n))
    k = max(text) + 1
    return craft(f"filler{n}_{v}", text, (lambda s: caterpillar(s, "right")) if k > 1 else (lambda s: s[0]), k)


CASES: dict[str, Callable[[], Case]] = {}
LONG_CASES = [f"cat{d}_{side}" for d in LONG_DEPTHS for side in SIDES]
for _d in LONG_DEPTHS:
    for _s in SIDES:
        CASES[f"cat{_d}_{_s}"] = functools.partial(_long, _d, _s)
LIMIT_CASE = "cat65_right"  # one bit past what the GPU decoder admits
CASES[LIMIT_CASE] = functools.partial(_long, 65, "right")
DEEP_CASE = "cat100_alt"  # far past it: the oracle and the host decoder still read it
CASES[DEEP_CASE] = functools.partial(_long, 100, "alt")
CASES["stride3"] = _stride3
CASES["complete8_100k"] = _complete8
NOSYNC_CASES = ["stride3", "complete8_100k"]
EDGE_CASES = ["complete256_8192", "two_leaf_24576", "two_leaf_24577", "two_leaf_8191", "single_1", "single_4097",
              "unused_leaves"]
CASES["complete256_8192"] = _complete256
for _n in (24576, 24577, 8191):
    CASES[f"two_leaf_{_n}"] = functools.partial(_two_leaf, _n)
for _n in (1, 4097):
    CASES[f"single_{_n}"] = functools.partial(_single, _n)
CASES["unused_leaves"] = _unused_leaves
LF_CASES = [f"lf_n{n}_p{p}" for n in LF_SIZES for p in lf_primaries(n)]
for _n in LF_SIZES:
    for _p in lf_primaries(_n):
        CASES[f"lf_n{_n}_p{_p}"] = functools.partial(_lf_case, _n, _p)
LF_BIG_CASE = f"lf_big_{LF_BIG_N}"
CASES[LF_BIG_CASE] = lambda: encoded(LF_BIG_CASE, random_text(300, LF_BIG_N, 256))
PERIODIC_CASES = [f"per_u{u}_k{k}_r{r}" for u, k, ranks in PERIODIC for r in ranks]
for _u, _k, _ranks in PERIODIC:
    for _r in _ranks:
        CASES[f"per_u{_u}_k{_k}_r{_r}"] = functools.partial(_periodic_case, _u, _k, _r)
FILLER_CASES = [f"filler{n}_{v}" for n in (1, 2, 3) for v in (0, 1)]
for _n in (1, 2, 3):
    for _v in (0, 1):
        CASES[f"filler{_n}_{_v}"] = functools.partial(_filler, _n, _v)

# every record the GPU tests decode (the limit and deep cases are refused there / host only)
GPU_CASES = LONG_CASES + NOSYNC_CASES + EDGE_CASES + LF_CASES + [LF_BIG_CASE] + PERIODIC_CASES + FILLER_CASES
ALL_CASES = GPU_CASES + [LIMIT_CASE, DEEP_CASE]


@functools.lru_cache(maxsize=None)
def get(name: str) -> Case:
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 2000))
    c = CASES[name]()
    assert c.name == name
    return c


def payload_offset(rec: bytes) -> int:
    return 24 + int.from_bytes(rec[16:24], "little")


def unaligned_batch(names=None) -> list[Case]:
    """The records of `names` (default: the long-code, never-resynchronising, edge, LF and
    periodic cases) back to back, with 1- to 3-byte blocks put in between until the record
    offsets and the output offsets have taken every residue mod 16 (so every residue mod 4 too)
    and the payloads every residue mod 4."""
    names = list(names or LONG_CASES + NOSYNC_CASES + EDGE_CASES + LF_CASES + [LF_BIG_CASE] + PERIODIC_CASES)
    fill = [get(f) for f in FILLER_CASES]
    out: list[Case] = []
    for i, nm in enumerate(names):
        out.append(get(nm))
        if i % 4 == 3:
            out.append(fill[(i // 4) % len(fill)])
    for i in range(256):
        if all(len(s) == m for s, m in zip(batch_residues(out), (16, 16, 4))):
            return out
        out.append(fill[i % len(fill)])
    raise AssertionError("unaligned batch: residues not covered")


def batch_residues(cases) -> tuple[set, set, set]:
    """Residues taken by the record offsets (mod 16), output offsets (mod 16) and payload
    offsets (mod 4) of records laid back to back."""
    ro = oo = 0
    r16, o16, p4 = set(), set(), set()
    for c in cases:
        r16.add(ro % 16)
        o16.add(oo % 16)
        p4.add((ro + payload_offset(c.rec)) % 4)
        ro += len(c.rec)
        oo += len(c.text)
    return r16, o16, p4
