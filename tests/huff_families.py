"""Histogram families for the GPU code-book kernel (csrc/huffman.hip k_huff_build), and the
rounds restatement of test_huffman_queue.py instrumented to say which of the kernel's branches a
frequency vector reaches. A plain module, like record_craft.py: tests/test_huff_families.py checks
the families on the CPU (oracle, host build and restatement agree; the families reach what they
are for), tests/test_gpu_codebook.py feeds them to Context.codebook_dev.

A shape is a list of frequencies in first-occurrence (leaf) order. A case gives it symbol values,
first positions and a block size:
  * model-path cases: the shape times the smallest power of two that brings its sum to >= 2^17
    (ties are scale-invariant; below 2^17 the reference's heap history may decide the order), the
    sum being the block size;
  * top-of-range cases: the largest frequencies a block can carry (multi-GiB block sizes);
  * heap-history cases: block sizes of the golden bands and leaf counts at which bmh.node_ranks
    reports the heap history, with frequencies that sum exactly to the size.
Variant 0 keeps symbol = leaf id and first = 0..L-1; the others draw the symbol values and the
first positions from a seeded generator, so a leaf id is not its symbol and the positions are
scattered over the block.
"""
from __future__ import annotations

import heapq
import os
import sys
from functools import lru_cache
from typing import NamedTuple

import numpy as np

import bmh
from oracle_ffi import REPO
from test_huffman_queue import _addr_rank, _internal_rank

sys.path.insert(0, os.path.join(REPO, "oracle", "alloc_trace"))
import band_trace  # noqa: E402  (test infrastructure: the glibc heap restatement)

BAND_CEIL = 1 << 17  # csrc/bmh_internal.h kBandCeil
M64 = (1 << 64) - 1


class Case(NamedTuple):
    name: str
    kind: str          # "model" | "top" | "history"
    n: int             # block size = sum of the frequencies
    freq: np.ndarray   # uint64[256], by symbol
    first: np.ndarray  # uint64[256], by symbol (UINT64_MAX where absent)

    @property
    def leaves(self) -> int:
        return int(np.count_nonzero(self.freq))


def fib(k: int) -> list[int]:
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


# ---------------------------------------------------------------------------- shapes
EQUAL_L = [1, 2, 3, 63, 64, 65, 127, 128, 129, 130, 192, 193, 194, 255, 256]
RANDOM_RANGES = [1, 2, 3, 5, 40]
RANDOM_L = [129, 200, 256]


def shapes() -> dict[str, list[int]]:
    s: dict[str, list[int]] = {}
    for L in EQUAL_L:  # the edges of addr_rank / internal_rank and of the 64-node words
        s[f"equal{L}"] = [1] * L
    s["two_level_128x1_128x2"] = [1] * 128 + [2] * 128
    s["two_level_200x3_56x1000"] = [3] * 200 + [1000] * 56
    s["staircase"] = [1 + i // 4 for i in range(256)]
    s["arith_up"] = list(range(1, 257))
    s["arith_down"] = list(range(256, 0, -1))
    s["heavy_255equal"] = [100_000] + [3] * 255
    s["pow2_runs8"] = [1 << (i // 8) for i in range(136)]  # 17 runs: L > 128, sum 8 (2^17 - 1)
    s["fib30_200equal"] = fib(30) + [1000] * 200
    s["fib45"] = fib(45)
    s["fib40_reversed"] = fib(40)[::-1]
    rng = np.random.default_rng(7)  # small ranges: long runs of equal frequencies
    for hi in RANDOM_RANGES:
        for L in RANDOM_L:
            s[f"random_hi{hi}_L{L}"] = [int(v) for v in rng.integers(1, hi + 1, L)]
    return s


VARIANTS = 3


def make_case(name: str, kind: str, leaf_freq: list[int], n: int, variant: int) -> Case:
    L = len(leaf_freq)
    assert 1 <= L <= 256 and sum(leaf_freq) == n and min(leaf_freq) >= 1 and L <= n, name
    if variant == 0:
        syms, pos = np.arange(L), np.arange(L)
    else:
        import zlib
        rng = np.random.default_rng([zlib.crc32(name.encode()), variant])
        syms = rng.permutation(256)[:L]
        if n <= 4096:
            pos = np.sort(rng.permutation(n)[:L])
        else:
            pos = np.unique(rng.integers(0, n, 4 * L + 16))
            assert pos.size >= L
            pos = np.sort(rng.permutation(pos)[:L])
    freq = np.zeros(256, np.uint64)
    first = np.full(256, M64, np.uint64)
    freq[syms] = np.array(leaf_freq, np.uint64)
    first[syms] = pos.astype(np.uint64)  # ascending with the leaf id
    return Case(f"{name}/v{variant}", kind, n, freq, first)


def model_scale(total: int) -> int:
    k = 1
    while total * k < BAND_CEIL:
        k *= 2
    return k


@lru_cache(maxsize=None)
def all_model_cases() -> tuple[Case, ...]:
    out = []
    for name, f in shapes().items():
        k = model_scale(sum(f))
        lf = [v * k for v in f]
        for v in range(VARIANTS):
            out.append(make_case(name, "model", lf, sum(lf), v))
    return tuple(out)


BATCH_MAX_N = 16 << 20


def model_cases() -> tuple[Case, ...]:
    """The model-path cases small enough to stand in one batch with an output buffer."""
    return tuple(c for c in all_model_cases() if c.n <= BATCH_MAX_N)


def big_model_cases() -> tuple[Case, ...]:
    """The Fibonacci chains (hundreds of MiB to GiB): calls without an output buffer."""
    return tuple(c for c in all_model_cases() if c.n > BATCH_MAX_N)


@lru_cache(maxsize=None)
def top_cases() -> tuple[Case, ...]:
    """The largest-frequency end: freq << 32 keys and the u32 sums of internal frequencies. Each
    is meant for a call of its own without an output buffer (the payload would be GiBs)."""
    a = [1 << 31, (1 << 31) - 2]  # 4 294 967 294: the largest block a batch admits
    b = fib(45)                   # 2 971 215 072, depth 44
    return (make_case("top_2p31_pair", "top", a, sum(a), 1), make_case("top_fib45", "top", b, sum(b), 1))


HISTORY_N = [17, 100, 256, 4250, 10000, 42000, 63800]


@lru_cache(maxsize=None)
def history_leaf_counts(n: int) -> tuple[int, ...]:
    """Leaf counts of an n-byte block at which the reference's heap history decides the node
    order: the smallest, the largest, 128 / 129 / 256 where admitted, and one in between."""
    hist = [L for L in range(1, min(n, 256) + 1) if bmh.node_ranks(n, L)[1]]
    if not hist:
        return ()
    pick = {hist[0], hist[-1], hist[len(hist) // 2]} | ({128, 129, 256} & set(hist))
    return tuple(sorted(pick))


def near_equal(n: int, L: int) -> list[int]:
    return [n // L + (1 if i < n % L else 0) for i in range(L)]


def staircase_topped(n: int, L: int) -> list[int]:
    """The steepest staircase 1 + i // k (k = 4, 8, ...) whose sum fits n, the rest on one leaf."""
    k = 4
    while sum(1 + i // k for i in range(L)) > n:
        k *= 2
    f = [1 + i // k for i in range(L)]
    f[L // 2] += n - sum(f)
    return f


def fib_then_equal(n: int, L: int) -> list[int]:
    """The longest Fibonacci prefix that leaves every other leaf at least one count, then a
    near-equal split of what remains."""
    k = 0
    while k + 1 < L and sum(fib(k + 1)) + (L - k - 1) <= n:
        k += 1
    pre = fib(k) if k else []
    return pre + near_equal(n - sum(pre), L - k)


HISTORY_SHAPES = {"near_equal": near_equal, "staircase": staircase_topped, "fib_equal": fib_then_equal}


@lru_cache(maxsize=None)
def history_cases() -> tuple[Case, ...]:
    out = []
    for n in HISTORY_N:
        for L in history_leaf_counts(n):
            for v, (sname, fn) in enumerate(HISTORY_SHAPES.items()):
                out.append(make_case(f"hist_n{n}_L{L}_{sname}", "history", fn(n, L), n, 1 + v % 2))
    return tuple(out)


# ---------------------------------------------------------------------------- tables from a tree
def leaf_order(freq, first) -> list[int]:
    return sorted((s for s in range(256) if freq[s]), key=lambda s: int(first[s]))


def tables_from_kids(order: list[int], kids: dict[int, tuple[int, int]]):
    """(len[256], code[256], tree bytes, depth) of the tree with leaves 0..L-1 (symbols `order`)
    and internal nodes L.. (kids: first pop = left = 0, second = right = 1; the root is the last):
    traverse (main.cpp:132-147) and the preorder bits of tree_to_bytes (:174-196)."""
    L = len(order)
    ln, code, bits = [0] * 256, [0] * 256, []
    stack = [(2 * L - 2, 0, 0)]
    depth = 0
    while stack:  # preorder, left before right
        v, c, d = stack.pop()
        if v < L:
            ln[order[v]], code[order[v]] = d, c
            depth = max(depth, d)
            bits.append("0" + format(order[v], "08b"))
        else:
            bits.append("1")
            a, b = kids[v]
            stack.append((b, (c << 1) | 1, d + 1))
            stack.append((a, c << 1, d + 1))
    s = "".join(bits)
    s += "0" * (-len(s) % 8)
    return ln, code, bytes(int(s[i:i + 8], 2) for i in range(0, len(s), 8)), depth


def payload_bytes(freq, ln) -> int:
    """encode_with_huffman (main.cpp:158-172): max(1, ceil(bits / 8))."""
    bits = sum(int(freq[s]) * ln[s] for s in range(256))
    return max(1, (bits + 7) // 8)


@lru_cache(maxsize=None)
def _trace_ranks(n: int, L: int) -> tuple[int, ...]:
    return tuple(band_trace.node_ranks(n, L))


def priority_queue_tables(freq, first, n: int):
    """A plain priority queue: pops the smallest frequency, among equals the node with the higher
    address rank (main.cpp:232-253 under band_trace's restatement of the glibc heap)."""
    order = leaf_order(freq, first)
    L = len(order)
    rank = _trace_ranks(n, L)
    heap = [(int(freq[order[i]]), -rank[i], i) for i in range(L)]
    heapq.heapify(heap)
    kids = {}
    for v in range(L, 2 * L - 1):
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        kids[v] = (a[2], b[2])
        heapq.heappush(heap, (a[0] + b[0], -rank[v], v))
    return tables_from_kids(order, kids)[:3]


# ---------------------------------------------------------------------------- the restatement
class Rounds(NamedTuple):
    len: list          # code length by symbol
    code: list         # code word by symbol
    tree: bytes        # preorder tree bytes
    depth: int
    rounds: int
    bound_rounds: int
    heap_steps: int
    largest_group: int       # most internal nodes of one frequency among the known nodes of a round
    groups: int              # distinct frequency groups of the finished tree's internal nodes
    span_groups: int         # (round, group) pairs whose group lies in more than one 64-node word
    wide_groups: int         # (round, group) pairs whose group is wider than 64 nodes
    lookups: int             # node_of calls
    lookups_63: tuple        # sorted-internal indices x with x % 64 == 63 that were looked up
    back_steps: int          # steps of node_of's backward search over gm[] words
    fwd_found_later: int     # lookups whose group end was found in a later gm[] word
    crossed_empty_word: int  # lookups that stepped over a gm[] word with no start bit


def instrumented_rounds(freq, first) -> Rounds:
    """parallel_rounds_lengths of test_huffman_queue.py (the round form k_huff_build runs on the
    closed-form order), with the kernel's own bookkeeping restated beside it: the four 64-bit
    group-start masks gm[] and node_of's searches over them, checked on every lookup against the
    plain definition (sorted internal index x -> its frequency group reversed)."""
    import bisect
    order = leaf_order(freq, first)
    L = len(order)
    if L == 1:
        ln, code, tree, depth = tables_from_kids(order, {})
        return Rounds(ln, code, tree, depth, 0, 0, 0, 0, 0, 0, 0, 0, (), 0, 0, 0)
    A = sorted((int(freq[order[i]]) << 32) | ((0xFFFF - _addr_rank(L, i)) << 16) | i for i in range(L))
    F, kids, P = [], {}, []
    rmax = _internal_rank(L, 2 * L - 2)
    st = {"back": 0, "fwd": 0, "empty": 0, "n": 0}
    l63 = set()
    gm = [0, 0, 0, 0]

    def ikey(j):
        return (F[j] << 32) | ((0xFFFF - _internal_rank(L, L + j)) << 16) | (L + j)

    def node_of(x, m, srt):
        q, r = x >> 6, x & 63
        w = gm[q] & (M64 if r == 63 else (2 << r) - 1)
        t = 0
        while t < 3 and not w and q > 0:
            q -= 1
            w = gm[q]
            t += 1
        st["back"] += t
        empty = t >= 2
        gs = 64 * q + w.bit_length() - 1
        q = x >> 6
        w = 0 if r == 63 else gm[q] & ~((2 << r) - 1) & M64
        t = 0
        while t < 3 and not w and q < 3:
            q += 1
            w = gm[q]
            t += 1
        if w and t:
            st["fwd"] += 1
            empty |= t >= 2
        ge = 64 * q + ((w & -w).bit_length() - 1) if w else m
        st["empty"] += empty
        st["n"] += 1
        if r == 63:
            l63.add(x)
        node = gs + ge - 1 - x
        assert node == srt[x], (x, m, node, srt[x])
        return node

    def sorted_internals(m):
        out, j = [], 0
        while j < m:
            e = j
            while e < m and F[e] == F[j]:
                e += 1
            out += list(range(e - 1, j - 1, -1))
            j = e
        return out

    m = lc = ic = rounds = bounds = 0
    largest = span = wide = 0
    while m + 1 < L:
        rounds += 1
        srt = sorted_internals(m)
        bound = False
        if m:
            B = (F[m - 1] << 32) | ((0xFFFF - rmax) << 16)
            la = bisect.bisect_left(A, B)
            ia = sum(1 for j in range(m) if F[j] < F[m - 1])
            bound = la + ia >= 2 * m + 2
        if bound:
            bounds += 1
            new = sorted(A[lc:la] + [ikey(node_of(x, m, srt)) for x in range(ic, ia)])
            P[lc + ic:] = new
            lc, ic = la, ia
        else:
            while lc + ic < 2 * m + 2:
                a = A[lc] if lc < L else 1 << 64
                c = ikey(node_of(ic, m, srt)) if ic < m else 1 << 64
                P[lc + ic:lc + ic + 1] = [min(a, c)]
                if a < c:
                    lc += 1
                else:
                    ic += 1
        m2 = min((lc + ic) // 2, L - 1)
        for j in range(m, m2):
            a, c = P[2 * j], P[2 * j + 1]
            F.append((a >> 32) + (c >> 32))
            kids[L + j] = (a & 0xFFFF, c & 0xFFFF)
        m = m2
        gm = [0, 0, 0, 0]
        j = 0
        while j < m:  # the groups among the known nodes, as the kernel's ballots see them
            gm[j >> 6] |= 1 << (j & 63)
            e = j
            while e < m and F[e] == F[j]:
                e += 1
            largest = max(largest, e - j)
            span += (j >> 6) != ((e - 1) >> 6)
            wide += e - j > 64
            j = e
    assert F == sorted(F) and max(F) < 1 << 32  # the kernel keeps F in u32
    ln, code, tree, depth = tables_from_kids(order, kids)
    return Rounds(ln, code, tree, depth, rounds, bounds, rounds - bounds, largest, len(set(F)), span, wide, st["n"],
                  tuple(sorted(l63)), st["back"], st["fwd"], st["empty"])


# ---------------------------------------------------------------------------- references
def reference_tables(case: Case, oracle):
    """(len[256], code[256], tree bytes) a block of this histogram and size must get: the oracle's
    tree on the closed-form order (sizes from 2^17), the plain priority queue on the heap-history
    ranks below."""
    if case.n >= BAND_CEIL:
        ln, code, tree = oracle.huffman_build(case.freq, case.first)
        return [int(v) for v in ln], [int(v) for v in code], tree
    return priority_queue_tables(case.freq, case.first, case.n)
