"""fp32 numpy restatement of torch.nn.utils.clip_grad_norm_ (L2, error_if_nonfinite=False) for the three optimizer
groups of the IQL step (ImplicitQLearning.set_grad_clip), over the oracle's gradient dict
{net: {tensor: array}}.  Not a test module."""
import numpy as np

GROUPS = {"vf": ("vf",), "qf": ("q1", "q2"), "actor": ("pi",)}
ORDER = ("vf", "qf", "actor")
EPS = np.float32(1e-6)


def no_limit(m):
    return m is None or not m > 0 or m == float("inf")


def coef(norm, max_norm):
    """min(max_norm / (norm + 1e-6), 1) in fp32; exactly 1 without a limit."""
    if no_limit(max_norm):
        return np.float32(1.0)
    return np.float32(min(np.float32(max_norm) / (np.float32(norm) + EPS), np.float32(1.0)))


def tensor_norm(g, lanes=8):
    """fp32 L2 norm of one tensor in the order torch's CPU kernel uses for a contiguous fp32 tensor: `lanes` running
    fp32 sums of fused x * x + acc over the elements i = lane (mod lanes), added up lane by lane, then the tail.  A
    plainly ordered or float64 sum of the 65 536 squares of a hidden layer's weight gradient sits up to 12 ulp away
    from torch's value (measured on the oracle's gradients), so the restatement follows torch's order; the products
    are exact in float64 and each sum is rounded to fp32 once, as a fused multiply-add does.
    Assumption (tests/test_grad_clip_cpu.py sets it): torch reduces the tensor in ONE thread (torch.set_num_threads(1))
    with 8 fp32 accumulators, what its CPU kernels use on AVX2 and on AVX-512 hosts alike; a torch build that reduces
    in another order differs from this restatement by that order's rounding only."""
    x = np.asarray(g, dtype=np.float32).ravel().astype(np.float64)
    n = x.size // lanes * lanes
    acc = np.zeros(lanes, dtype=np.float32)
    for row in x[:n].reshape(-1, lanes):
        acc = (acc.astype(np.float64) + row * row).astype(np.float32)
    s = np.float32(0.0)
    for a in acc:
        s = np.float32(s + a)
    for v in x[n:]:
        s = np.float32(np.float64(s) + v * v)
    return np.float32(np.sqrt(s))


def group_norm(grads, nets):
    """fp32 total norm as torch forms it: the fp32 norm of the tensors' fp32 norms."""
    per = np.array([tensor_norm(g) for n in nets for g in grads[n].values()], dtype=np.float32)
    return tensor_norm(per)


def clip_coefs(grads, max_norm):
    """max_norm: {"vf" | "qf" | "actor": limit or None}.  Returns (scaled gradient dict, {group: norm}, {group: coef})."""
    norms, coefs = {}, {}
    out = {n: dict(t) for n, t in grads.items()}
    for grp in ORDER:
        nets = GROUPS[grp]
        norms[grp] = group_norm(grads, nets)
        coefs[grp] = coef(norms[grp], max_norm.get(grp))
        for n in nets:
            out[n] = {k: (g.astype(np.float32) * coefs[grp]).astype(np.float32) for k, g in grads[n].items()}
    return out, norms, coefs
