"""CPU checks of the case table tests/chunk_kind_shapes.py: what it states per shape (layer-0 staging, row width) against
helpers' restatements of the host's rules, and that its cases reach every instantiation of the five training forwards
and every row stride they are there for.  Nothing is measured and nothing runs on a device: these are conditions on the
table, so that a cell dropped from it later to save time cannot silently drop an instantiation."""
import chunk_kind_shapes as T
from helpers import (CHUNK_KINDS, bwd_instantiation, fwd_instantiation, fwd_spb_l2, row_f4, train_steps_decomposition,
                     uses_large_batch_kernels, w0_lds_k)


def _cases(**want):
    keys = ("kind", "S", "A", "gaussian", "B", "precision")
    return [c for c in T.CASES if all(c[keys.index(k)] == v for k, v in want.items())]


def test_the_table_states_each_shapes_staging_and_row_width():
    assert len({(S, A) for S, A, *_ in T.DIMS}) == len(T.DIMS) == 6
    for S, A, _, w0k, f4 in T.DIMS:
        assert S + A <= 128 and 1 <= A <= 32
        assert (w0_lds_k(S, A), row_f4(S, A)) == (w0k, f4), (S, A, w0_lds_k(S, A), row_f4(S, A))
    staged = {(S, A): w0k for S, A, _, w0k, _ in T.DIMS}
    # every instance staged (kq fits) / only V and pi (S fits, kq does not) / none, on both sides of the LDS-DMA switch
    assert staged[(39, 28)] == 39 + 28 > 64 and staged[(72, 28)] == 72 > 64             # W0DMA = 1: all / split
    assert staged[(17, 6)] == 17 + 6 <= 64 and staged[(64, 32)] == 64                    # W0DMA = 0: all / split
    assert staged[(100, 28)] == staged[(127, 1)] == 0
    assert T.DIMS_OF[(64, 32)][0] is False and all(g for (S, A), (g, _, _) in T.DIMS_OF.items() if (S, A) != (64, 32))


def test_127_1_is_the_only_stride_above_256_floats():
    """S + A <= 128 and A >= 1: the stride 2 S + A + 2 = S + (S + A) + 2 <= 127 + 128 + 2 = 257, reached by S = 127 alone;
    every other admissible shape has at most 256 floats, 64 float4: one pass of a wave's row loop and at most
    32 * 64 / 256 = 8 xr registers."""
    wide = [(S, A) for S in range(1, 128) for A in range(1, 33) if S + A <= 128 and row_f4(S, A) > 64]
    assert wide == [(127, 1)] and row_f4(127, 1) == 65
    assert -(-32 * row_f4(127, 1) // 256) == 9 and -(-32 * row_f4(100, 28) // 256) == 8
    assert max(row_f4(S, A) for S in range(1, 128) for A in range(1, 33) if S + A <= 128 and (S, A) != (127, 1)) == 64


def test_batch_sizes_take_the_paths_the_table_names():
    assert [fwd_spb_l2((B + 31) // 32) for B in (40, 300, 600)] == [0, 1, 2]
    assert 40 % 32 and 300 % 32 and 600 % 32                                  # every batch ends in a ragged row tile
    assert "FULL=0" in bwd_instantiation(17, 6, 300, "f32") and (300 + 255) // 256 == 2
    assert train_steps_decomposition(T.CALLS[0]) == (2, [4, 1])               # a direct head + two chunk graphs
    assert T.CALLS[1] == 3 and T.CALLS[-2] % 2 == 0                           # the last call follows an even one
    for B in (40, 300, 600):
        assert 1 <= T.n_off_of(B) <= B - 1 and T.n_off_of(B) % 2 == 1 and B % 2 == 0
    assert T.N_ONLINE < T.ONLINE_CAPACITY and T.N_ROWS == 2000


def test_every_forward_instantiation_is_named_by_a_case():
    want = T.all_instantiations()
    assert len(want) == len(set(want)) == 32
    named = {T.instantiation(c) for c in T.CASES}
    missing = [n for n in want if n not in named]
    assert not missing, f"no case runs {missing}"
    extra = sorted(named - set(want))
    assert not extra, f"cases outside the chunk kinds' training forwards: {extra}"
    assert len(T.CASES) == len(set(T.CASES)) == len({T.case_id(c) for c in T.CASES})


def test_every_kind_runs_every_shape_in_fp32():
    missing = [(k, S, A) for k in CHUNK_KINDS for S, A, *_ in T.DIMS
               if not [c for c in _cases(kind=k, S=S, A=A, precision="f32") if c[4] in (40, 300)]]
    assert not missing, f"no fp32 case at 40 or 300 rows for {missing}"
    for c in T.CASES:
        assert c[3] == T.DIMS_OF[(c[1], c[2])][0], c


def test_every_kind_runs_the_widest_row_at_both_batch_sizes():
    missing = [(k, B) for k in CHUNK_KINDS for B in (40, 300) if not _cases(kind=k, S=127, A=1, B=B, precision="f32")]
    assert not missing, f"(127, 1) is not run for {missing}"


def test_600_rows_run_for_every_kind_at_39_28_only():
    big = [c for c in T.CASES if c[4] > 300]
    assert {c[4] for c in big} == {600} and {(c[1], c[2], c[5]) for c in big} == {(39, 28, "f32")}
    missing = [k for k in CHUNK_KINDS if not _cases(kind=k, B=600)]
    assert not missing, f"no 600-row case for {missing}"
    # today's shape stays only above 256 rows (where the earlier mixed and weighted tests never went)
    assert {c[4] for c in _cases(S=17, A=6)} == {300}


def test_bf16_cases_reach_every_bf16_forward():
    bf = _cases(precision="bf16")
    assert {c[0] for c in bf} == set(T.BF16_KINDS) == {"plain", "mixed", "weighted"}
    for c in bf:
        assert c[4] <= 512 and not uses_large_batch_kernels(c[1], c[2], c[4]), c
    want = [n for n in T.all_instantiations() if "BF16=1" in n]
    assert len(want) == 12
    named = {T.instantiation(c) for c in bf}
    missing = [n for n in want if n not in named]
    assert not missing, f"no bf16 case runs {missing}"


def test_fwd_instantiation_follows_the_cu_count_and_the_large_batch_switch():
    assert fwd_instantiation("plain", 17, 6, 256, "f32") == "iql_fwd_kernel<BF16=0, W0DMA=0, MULTI=0>"
    assert fwd_instantiation("plain", 17, 6, 256, "f32", n_cus=128) == "iql_fwd_kernel<BF16=0, W0DMA=0, MULTI=1>"
    assert fwd_instantiation("weighted", 39, 28, 300, "bf16") == "iql_fwd_weighted_kernel<BF16=1, W0DMA=1, MULTI=1>"
    assert fwd_instantiation("prioritized", 72, 28, 40, "f32") == "iql_fwd_prio_kernel<W0DMA=1, MULTI=0>"
    assert fwd_instantiation("weighted_is", 127, 1, 300, "f32") == "iql_fwd_weighted_is_kernel<W0DMA=0, MULTI=1>"
    assert fwd_instantiation("plain", 39, 28, 600, "bf16") == "iql_fwd_lb_kernel<NKB=3>"
    assert fwd_instantiation("plain", 100, 28, 600, "bf16") == "iql_fwd_kernel<BF16=1, W0DMA=0, MULTI=1>"
