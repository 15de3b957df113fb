"""The histogram families of tests/huff_families.py on the CPU: the references the GPU code-book
test (tests/test_gpu_codebook.py) compares the kernel with agree with each other on every case,
and the families reach the branches of k_huff_build they were made for (csrc/huffman.hip: groups
of internal nodes wider than a 64-node word, sorted-internal indices on a word's last bit, pure
heap-order chains, many small groups, the u32 top of the frequency range, the heap-history order).
The figures asserted here are properties of the fixtures, as the instrumented restatement counts
them; re-derive them when a shape changes."""
import numpy as np

import bmh
import huff_families as hf


def _host(c: hf.Case):
    t = bmh.huffman_build(c.freq, c.first, c.n)
    return list(t.len), list(t.code), t.tree_bytes, t.tree_len, t.leaves


def test_case_shapes_are_well_formed():
    names = set()
    for c in hf.all_model_cases() + hf.top_cases() + hf.history_cases():
        assert c.name not in names
        names.add(c.name)
        present = np.flatnonzero(c.freq)
        assert int(c.freq.sum()) == c.n and 1 <= present.size <= 256
        pos = c.first[present]
        assert len(set(pos.tolist())) == present.size and int(pos.max()) < c.n
        assert (c.first[c.freq == 0] == hf.M64).all()
    assert all(c.n >= hf.BAND_CEIL for c in hf.all_model_cases() + hf.top_cases())
    assert [c.n for c in hf.top_cases()] == [4_294_967_294, 2_971_215_072]
    # permuted variants: a leaf id is not its symbol, first positions are not 0..L-1
    for c in hf.all_model_cases():
        if c.name.endswith("/v0") or c.leaves < 3:
            continue
        order = hf.leaf_order(c.freq, c.first)
        assert order != sorted(order), c.name
        assert sorted(int(c.first[s]) for s in order) != list(range(len(order))), c.name
    assert len(hf.model_cases()) + len(hf.big_model_cases()) == len(hf.all_model_cases()) == 3 * len(hf.shapes())
    assert len(hf.model_cases()) >= 100 and sum(c.n for c in hf.model_cases()) < 64 << 20


def test_model_path_references_agree(oracle):
    """Oracle, host build and the rounds restatement give the same lengths, codes and tree bytes
    on every model-path and top-of-range case, and the closed-form order is what applies there."""
    for c in hf.all_model_cases() + hf.top_cases():
        oln, ocode, otree = oracle.huffman_build(c.freq, c.first)
        ref = ([int(v) for v in oln], [int(v) for v in ocode], otree)
        r = hf.instrumented_rounds(c.freq, c.first)
        assert (r.len, r.code, r.tree) == ref, c.name
        assert _host(c)[:3] == ref, c.name
        assert hf.reference_tables(c, oracle) == ref, c.name
        L = c.leaves
        ranks, from_history = bmh.node_ranks(c.n, L)
        assert not from_history and ranks == hf.band_trace.model_ranks(L), c.name
        assert _host(c)[3:] == ((10 * L - 1 + 7) // 8, L), c.name


def _rounds(shape: str) -> hf.Rounds:
    c = next(c for c in hf.all_model_cases() if c.name == shape + "/v0")
    return hf.instrumented_rounds(c.freq, c.first)


def test_families_reach_the_kernel_branches():
    rs = {c.name: hf.instrumented_rounds(c.freq, c.first) for c in hf.model_cases()}
    # a group wider than 64 nodes leaves a gm[] word without a start bit: node_of's backward and
    # forward searches step over it
    assert any(r.wide_groups for r in rs.values())
    assert any(r.crossed_empty_word for r in rs.values())
    assert sum(r.back_steps > 0 for r in rs.values()) >= 30
    assert sum(r.fwd_found_later > 0 for r in rs.values()) >= 30
    # sorted-internal indices on the last bit of each word ((x & 63) == 63)
    assert {x for r in rs.values() for x in r.lookups_63} == {63, 127, 191}
    r = _rounds("equal256")
    assert (r.rounds, r.largest_group, r.depth) == (15, 128, 8) and r.wide_groups == 14
    assert r.crossed_empty_word > 0
    r = _rounds("staircase")
    assert r.groups == 181 > 150 and r.largest_group == 3
    r = _rounds("two_level_200x3_56x1000")
    assert (r.rounds, r.largest_group, r.wide_groups) == (26, 100, 25)
    r = _rounds("fib30_200equal")
    assert r.largest_group == 99 and r.wide_groups == 17 and r.heap_steps == 15 and r.depth == 24
    # chains: every new node is popped next, so every round is a heap-order step
    r = _rounds("fib45")
    assert (r.rounds, r.heap_steps, r.bound_rounds, r.depth) == (44, 44, 0, 44)
    r = _rounds("fib40_reversed")
    assert (r.heap_steps, r.bound_rounds, r.depth) == (39, 0, 39)
    r = _rounds("pow2_runs8")
    assert r.heap_steps == 20 and r.bound_rounds == 19 and r.depth == 20
    # both classes of the address-rank model, and the smallest trees
    assert {c.leaves for c in hf.model_cases()} >= set(hf.EQUAL_L)
    top = [hf.instrumented_rounds(c.freq, c.first) for c in hf.top_cases()]
    assert [(t.rounds, t.depth) for t in top] == [(1, 1), (44, 44)]


def test_heap_history_cases(oracle):
    """Below 2^17 bytes the host build follows the reference's heap history: on every such case
    it equals a plain priority queue popping by (frequency, higher band_trace rank first)."""
    cases = hf.history_cases()
    hist = differs = 0
    for c in cases:
        L = c.leaves
        ranks, from_history = bmh.node_ranks(c.n, L)
        assert ranks == list(hf.band_trace.node_ranks(c.n, L)), c.name
        hist += from_history
        ref = hf.priority_queue_tables(c.freq, c.first, c.n)
        assert _host(c)[:3] == ref, c.name
        assert hf.reference_tables(c, oracle) == ref, c.name
        t0 = bmh.huffman_build(c.freq, c.first, 0)  # the closed-form order
        differs += (list(t0.len), list(t0.code), t0.tree_bytes) != ref
    assert hist == len(cases) >= 40
    assert {c.n for c in cases} == set(hf.HISTORY_N)
    for n in (256, 4250, 10000, 42000, 63800):
        assert {128, 129, 256} <= set(hf.history_leaf_counts(n)), n
    # the history is no formality: most of these tables differ from the closed form's
    assert differs >= len(cases) // 2, differs
    # several blocks of one size carry different histograms
    assert all(sum(1 for c in cases if c.n == n) >= 9 for n in hf.HISTORY_N)
