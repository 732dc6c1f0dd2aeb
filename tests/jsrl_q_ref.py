"""Plain numpy restatement of the JSRL critic selection (who == 3; include/iqlhip.h iqlhip_jsrl_act_q), on top of
oracle.philox_ref: the uniform of a row, the learner's probability, the decision with its tie rule, and the assembly
of the result.  Written from the header's rule, not from the kernels."""
import numpy as np

from oracle import philox_ref as P


def row_uniform(seed, call, rows, A):
    """u of rows 0 .. rows - 1 of one call: float32 [rows], the 24-bit unit float of word 2 of the act() noise
    stream's Philox block at element row * A (key = seed, counter = (element, lo32 call, hi32 call, 0xAC7))."""
    call = int(call) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = P._key(seed)
    e = np.arange(int(rows), dtype=np.uint64) * np.uint64(int(A))
    _, _, o2, _ = P.philox4x32_10(e, call & 0xFFFFFFFF, call >> 32, P.TAG_ACT, k0, k1)
    return P._unit24(o2)


def p_learner(ql, qg, inv_temp):
    """p = 1 / (1 + exp(-(ql - qg) * inv_temp)), every step in float32."""
    d = np.asarray(ql, np.float32) - np.asarray(qg, np.float32)
    with np.errstate(over="ignore"):
        x = np.exp((-d * np.float32(inv_temp)).astype(np.float32))
        return (np.float32(1.0) / (np.float32(1.0) + x)).astype(np.float32)


def q_min(q):
    """(qg, ql) of q [n, 4] = (Q1g, Q2g, Q1l, Q2l)."""
    q = np.asarray(q, np.float32)
    return np.minimum(q[:, 0], q[:, 1]), np.minimum(q[:, 2], q[:, 3])


def decide(q, inv_temp, seed=0, call=0, A=1):
    """use_learner [n] bool of rows whose byte is 3.  inv_temp infinite, or seed == 0: ql >= qg (a tie goes to the
    learner); else u < p."""
    qg, ql = q_min(q)
    if np.isinf(inv_temp) or int(seed) == 0:
        return ql >= qg
    return row_uniform(seed, call, len(qg), A) < p_learner(ql, qg, inv_temp)


def margin(q, inv_temp, seed, call, A):
    """|u - p| per row: how far a Boltzmann decision is from flipping."""
    qg, ql = q_min(q)
    return np.abs(row_uniform(seed, call, len(qg), A).astype(np.float64) - p_learner(ql, qg, inv_temp).astype(np.float64))


def assemble(a_guide, a_learner, use_learner):
    """The output rows: the chosen candidate, bit for bit."""
    return np.where(np.asarray(use_learner, bool)[:, None], a_learner, a_guide)
