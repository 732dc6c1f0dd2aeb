"""CPU companion of tests/test_hip_between_calls.py: the Python restatement of how iqlhip_train_steps composes a call
(tests/helpers.py: train_steps_decomposition, train_steps_graph_keys) against values worked by hand from
csrc/iqlhip.hip, the eviction case's key count, and — with the CPU restatement of the index draw, oracle/philox_ref.py —
the condition of the written-rows case: the row a single-row writer touches is in the first batch of the next call."""
import numpy as np
import pytest

from helpers import (GRAPH_CACHE_ENTRIES, SMALL_BUFFER, graph_cache_requests, train_steps_decomposition,
                     train_steps_graph_keys)
from oracle import philox_ref as R


@pytest.mark.parametrize("K,head,chunks", [
    (23, 2, [4, 16, 1]),            # n_chunks_for(19) = 16+2+1 = 3 is not below n_chunks_for(21) = 16+4+1 = 3: head 2
    (6, 2, [4]),                    # one chunk behind either head: 2
    (130, 2, [64, 64]),             # a head of 4 would leave 126 = 64 + 3*16 + 3*4 + 2 (8 chunks) instead of 2
    (1, 1, []), (2, 2, []), (3, 2, [1]),
    (4, 4, []),                     # nothing behind a head of 4, one chunk behind a head of 2
    (8, 4, [4]),                    # 4 behind a head of 4 is one chunk, 6 behind a head of 2 is two (4 + 2)
    (20, 4, [16]), (68, 4, [64]),
    (14, 2, [4, 4, 4]),
    (36, 4, [16, 16]),
    # 1020 behind a head of 4 = 15 * 64 + 3 * 16 + 3 * 4: 21 chunks; 1022 behind a head of 2 needs a 2-step chunk more
    (1024, 4, [4, 4, 4, 16, 16, 16] + [64] * 15),
])
def test_decomposition_matches_hand_worked_values(K, head, chunks):
    got = train_steps_decomposition(K)
    assert got == (head, chunks)
    assert got[0] + sum(got[1]) == K


def test_decomposition_covers_every_call_length():
    for K in range(1, 1025):
        head, chunks = train_steps_decomposition(K)
        assert head + sum(chunks) == K and head in (1, 2, 4) and (head == 1) == (K == 1)
        assert set(chunks) <= {1, 2, 4, 16, 64} and chunks.count(1) <= 1 and (not chunks or 1 not in chunks[:-1])
        # an even head and even chunks in front of the one-step chunk: every chunk's step 0 reads staging buffer 0
        assert all(c % 2 == 0 for c in chunks[:-1])


def test_graph_keys_of_the_issue_examples():
    assert [k[2] for k in train_steps_graph_keys(23, 64)] == [2, 4, 16, 1]
    assert [k[2] for k in train_steps_graph_keys(6, 256)] == [2, 4]
    assert [k[2] for k in train_steps_graph_keys(130, 256)] == [2, 64]
    a, b = train_steps_graph_keys(8, 256), train_steps_graph_keys(8, 256, drop_p=0.1)
    assert [k[2] for k in a] == [4] and a != b                     # the head's steps share the plain 4-step chunk
    assert train_steps_graph_keys(8, 256, rows=1) != a and train_steps_graph_keys(8, 256, stats=True) != a
    assert train_steps_graph_keys(8, 33)[0][4] == float(np.float32(1.0 / 33))


def test_eviction_case_requests_more_keys_than_the_cache_holds():
    """The GPU eviction case: batch sizes 32 .. 160 at 23 steps, three rounds.  20 distinct keys; the second and third
    round find none of theirs cached (LRU over a cycle longer than the cache): every request after the first 12
    evicts."""
    calls = [train_steps_graph_keys(23, B) for _ in range(3) for B in (32, 64, 96, 128, 160)]
    distinct, evictions = graph_cache_requests(calls)
    assert distinct == 20 > GRAPH_CACHE_ENTRIES
    assert evictions == 3 * 20 - GRAPH_CACHE_ENTRIES


def test_written_rows_are_in_the_first_batch_of_the_next_call():
    """Case 6's condition for its single-row writers, from the CPU index draw: the shim starts a call at counter
    total_it * ceil(B / 2)."""
    c = SMALL_BUFFER
    B, half = c["B"], (c["B"] + 1) // 2
    total_it = c["segments"][0]
    first = R.draw_indices(B, c["N"], c["seed"], total_it * half)
    assert c["pointer_row"] in first and c["reward_row"] in first
    assert len(set(first.tolist())) >= c["N"] - 2            # "almost every row"
