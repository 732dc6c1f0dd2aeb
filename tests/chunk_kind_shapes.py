"""The case table of tests/test_hip_chunk_kind_shapes.py (not a test module): every chunk-graph kind of train_steps at
every instantiation of its training forward and at the row strides at which a gather's loop over a row changes.

tests/test_chunk_kind_shapes_cpu.py checks the table's claims (staging rule, row width, instantiation names, coverage)
on the CPU; the GPU module runs the cases against each kind's eager twin, bit for bit."""
from helpers import CHUNK_KINDS, fwd_instantiation

# (S, A, gaussian, w0_lds_k, row_f4): the staging rule's result and the float4s of a packed row, stated here and checked
# against helpers' restatements of iqlhip_create's rule by the CPU test.
DIMS = [
    (17, 6, True, 23, 11),       # the shape of every earlier burst test: everything register-staged, one short row pass
    (39, 28, True, 67, 27),      # kq = 67: every instance staged by LDS-DMA
    (72, 28, True, 72, 44),      # kq = 100 > 96, S = 72 fits: V and pi by LDS-DMA, the critics stream W0 from global
    (64, 32, False, 64, 41),     # kq = 96 does not fit beside two head tiles: V and pi through registers, critics global
    (100, 28, True, 0, 58),      # nothing staged; the widest row of one pass per wave (58 of 64 lanes)
    (127, 1, True, 0, 65),       # the only stride above 256 floats: a second row pass, the forward's ninth xr register, A = 1
]
DIMS_OF = {(S, A): (gaussian, w0k, f4) for S, A, gaussian, w0k, f4 in DIMS}

# Rows per step.  40: a ragged pair of row tiles, fwd_spb_l2 = 0.  300: 10 row tiles, fwd_spb_l2 = 1, backward chunks of
# 256 + 44 rows.  600 (fp32 only: the bf16 entry points of the non-plain kinds refuse more than 512): fwd_spb_l2 = 2, the
# fewest idle blocks per row.
FP32_CELLS = [(17, 6, 300), (39, 28, 40), (39, 28, 600), (72, 28, 40), (72, 28, 300), (64, 32, 40), (100, 28, 300),
              (127, 1, 40), (127, 1, 300)]
# BF16 x W0DMA x MULTI for the three kinds that have bf16 forwards
BF16_CELLS = [(39, 28, 40), (72, 28, 300), (127, 1, 40), (127, 1, 300)]
BF16_KINDS = ("plain", "mixed", "weighted")

# Steps per call: 7 = a directly launched head of 2 + a 4-step and a 1-step chunk graph (helpers.
# train_steps_decomposition), so the set-up kernel's gather feeds step 0 and the idle blocks' gathers every later step,
# across two graph boundaries.  Then a second call of 3 steps, then 2 + 2: the last call follows an
# even one, which is the only way a call starts on rows the call before it staged (plain, weighted and weighted_is).
CALLS = (7, 3, 2, 2)
N_ROWS = 2000                    # rows of every buffer
N_ONLINE, ONLINE_CAPACITY = 300, 512      # the mixed kind's online buffer


def n_off_of(B):
    """Offline rows of a mixed batch of B: an odd count just under half."""
    return B // 2 - 3


def _case(kind, S, A, B, precision):
    return (kind, S, A, DIMS_OF[(S, A)][0], B, precision)


# (kind, S, A, gaussian, B, precision)
CASES = [_case(k, S, A, B, "f32") for k in CHUNK_KINDS for S, A, B in FP32_CELLS] + \
        [_case(k, S, A, B, "bf16") for k in BF16_KINDS for S, A, B in BF16_CELLS]


def case_id(c):
    kind, S, A, _, B, precision = c
    return f"{kind}-S{S}A{A}-B{B}-{precision}"


def instantiation(c, n_cus=256):
    kind, S, A, _, B, precision = c
    return fwd_instantiation(kind, S, A, B, precision, n_cus)


def all_instantiations():
    """The 32 names of the training forwards: 8 each for plain, mixed and weighted, 4 each for the fp32-only kinds."""
    out = []
    for name in ("iql_fwd_kernel", "iql_fwd_mixed_kernel", "iql_fwd_weighted_kernel"):
        out += [f"{name}<BF16={bf}, W0DMA={dma}, MULTI={multi}>" for bf in (0, 1) for dma in (0, 1) for multi in (0, 1)]
    for name in ("iql_fwd_weighted_is_kernel", "iql_fwd_prio_kernel"):
        out += [f"{name}<W0DMA={dma}, MULTI={multi}>" for dma in (0, 1) for multi in (0, 1)]
    return out
