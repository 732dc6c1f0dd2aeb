"""Weighted replay sampling: what a weight vector must look like and what the weighted calls refuse.

`ReplayBuffer.set_sample_weights(w)` attaches one float32 weight per row position to a GPU buffer; the library turns it
into a cumulative table of integers on the device (include/iqlhip.h "weighted replay sampling"), and
`draw_weighted_indices`, `sample_weighted` and `ImplicitQLearning.train_steps_weighted` draw rows by it from the index
stream of `train_steps`, unchanged.  Row i is drawn with probability q[i] / sum(q), q[i] = floor(w[i] * 2^(38 - e)),
e = floor(log2(max w)): a weight below max(w) * 2^-39 quantises to 0 and its row is never drawn.

Weights belong to row POSITIONS: writes into the buffer leave them alone; a change of the buffer's index bound makes the
weighted calls refuse until weights are set again.  Every other call (train_steps, sample, online_step, the groups'
other calls, mixed batches) ignores them.

`SampleWeights(w)` is the same table as an object of its own, bound to no buffer: K members of a trainer group that
share one buffer can each draw by a table of their own (`ImplicitQLearningGroup.train_steps_weighted(weights=[...])`),
and `ImplicitQLearning.train_steps_weighted(weights=...)` uses it instead of the buffer's.

Updatable tables (`set_sample_weights(w, updatable=True)`, `SampleWeights(w, updatable=True)`; DESIGN.md 6i "updatable
tables") can be changed in place, a few hundred rows in a few microseconds: `update_sample_weights(indices, weights)` /
`SampleWeights.update`.  Such a table spans the buffer's whole capacity, rows beyond the index bound weigh 0, and its
scale is fixed when it is built (`max_weight`), so the weighted calls keep working while the ring fills.

The argument checks live here, free of any GPU work, so they can be tested without one.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

MAX_ROWS = 1 << 24            # IQLHIP_WEIGHTS_MAX_ROWS (include/iqlhip.h)


def check_vector(weights, n: int):
    """The shape, dtype and length checks of set_sample_weights (no look at the values, which may live on the device):
    a 1-D float32 torch tensor or ndarray of n = the buffer's index bound entries, 1 <= n <= 2^24.  ValueError
    otherwise.  Returns "torch" or "numpy"."""
    import torch
    if n < 1:
        raise ValueError("iqlhip: the replay buffer is empty: there is no row to weigh")
    if n > MAX_ROWS:
        raise ValueError(f"iqlhip: weighted sampling covers at most 2^24 rows (the buffer draws over {n})")
    if isinstance(weights, torch.Tensor):
        kind, is_f32 = "torch", weights.dtype == torch.float32
    elif isinstance(weights, np.ndarray):
        kind, is_f32 = "numpy", weights.dtype == np.float32
    else:
        raise ValueError(f"iqlhip: sample weights must be a torch tensor or a numpy array, not {type(weights).__name__}")
    if not is_f32:
        raise ValueError(f"iqlhip: sample weights must be float32 (got {weights.dtype})")
    if weights.ndim != 1:
        raise ValueError(f"iqlhip: sample weights must be one-dimensional (got shape {tuple(weights.shape)})")
    if weights.shape[0] != n:
        raise ValueError(f"iqlhip: {weights.shape[0]} sample weights for a buffer that draws over {n} rows")
    return kind


def check_host_values(w: np.ndarray) -> None:
    """The value checks on a host vector (the library makes the same ones on the device): all finite, all >= 0, at
    least one > 0.  ValueError otherwise."""
    if not np.all(np.isfinite(w)):
        raise ValueError("iqlhip: sample weights hold a NaN or an infinity")
    if np.any(w < 0):
        raise ValueError("iqlhip: sample weights hold a negative value")
    if not np.any(w > 0):
        raise ValueError("iqlhip: all sample weights are zero")


def check_updatable_args(n: int, capacity, max_weight):
    """capacity and max_weight of an updatable table over n weights: n <= capacity <= 2^24 (None: n), max_weight finite
    and >= 0 (None or 0: the largest weight present).  Returns (capacity, max_weight); ValueError otherwise."""
    capacity = n if capacity is None else int(capacity)
    if capacity < n:
        raise ValueError(f"iqlhip: capacity {capacity} is smaller than the {n} sample weights")
    if capacity > MAX_ROWS:
        raise ValueError(f"iqlhip: weighted sampling covers at most 2^24 rows (capacity {capacity})")
    max_weight = 0.0 if max_weight is None else float(max_weight)
    if not (0.0 <= max_weight < float("inf")):
        raise ValueError(f"iqlhip: max_weight must be finite and not negative (got {max_weight})")
    return capacity, max_weight


def check_tracking_args(updatable: bool, track_max: bool, new_row_weight):
    """track_max / new_row_weight of a table: tracking belongs to an updatable table, new_row_weight (None: 1.0) is a
    finite float > 0 and means something only with track_max.  Returns new_row_weight (None without track_max);
    ValueError otherwise."""
    import math
    if not track_max:
        if new_row_weight is not None:
            raise ValueError("iqlhip: new_row_weight belongs to a table that tracks its maximum (track_max=True)")
        return None
    if not updatable:
        raise ValueError("iqlhip: track_max belongs to an updatable table (updatable=True)")
    try:
        w = 1.0 if new_row_weight is None else float(new_row_weight)
    except (TypeError, ValueError):
        raise ValueError(f"iqlhip: new_row_weight must be a number, not {type(new_row_weight).__name__}")
    if not math.isfinite(w) or w <= 0.0:
        raise ValueError(f"iqlhip: new_row_weight must be finite and > 0 (got {new_row_weight})")
    return w


def check_insert_args(row, bound, n: int) -> tuple:
    """(row, bound) of insert_max on a table over n rows: bound (None: n) in [0, n], row in [0, bound)."""
    bound = int(n) if bound is None else int(bound)
    if not 0 <= bound <= int(n):
        raise ValueError(f"iqlhip: bound {bound} outside [0, {n}]")
    row = int(row)
    if not 0 <= row < bound:
        raise ValueError(f"iqlhip: row {row} outside [0, {bound})")
    return row, bound


def online_offset_step(batch_size: int) -> int:
    """Philox counters the draw of one prioritised online step consumes: two indices per counter."""
    return (int(batch_size) + 1) // 2


def check_update_args(indices, weights, device=None) -> int:
    """The shape, dtype and device checks of an update: two 1-D device tensors of one length, int64 indices and float32
    weights (no look at the values: bad ones are skipped and flagged on the device).  Returns that length."""
    import torch
    if not isinstance(indices, torch.Tensor) or not isinstance(weights, torch.Tensor):
        raise ValueError("iqlhip: an update takes torch tensors (indices int64, weights float32)")
    if indices.dtype != torch.int64:
        raise ValueError(f"iqlhip: update indices must be int64 (got {indices.dtype})")
    if weights.dtype != torch.float32:
        raise ValueError(f"iqlhip: update weights must be float32 (got {weights.dtype})")
    if indices.ndim != 1 or weights.ndim != 1:
        raise ValueError("iqlhip: update indices and weights must be one-dimensional")
    if indices.shape[0] != weights.shape[0]:
        raise ValueError(f"iqlhip: {indices.shape[0]} update indices for {weights.shape[0]} weights")
    if device is not None and (indices.device != device or weights.device != device):
        raise ValueError(f"iqlhip: update indices and weights must live on the table's device ({device})")
    return int(indices.shape[0])


def check_td_args(indices, td, device=None) -> int:
    """The shape, dtype and device checks of an update by TD errors: int64 indices [m] and float32 TD errors [m, 2] (what
    trainer.last_td_errors() returns), device tensors (no look at the values).  Returns m."""
    import torch
    if not isinstance(indices, torch.Tensor) or not isinstance(td, torch.Tensor):
        raise ValueError("iqlhip: an update by TD errors takes torch tensors (indices int64, td float32 [m, 2])")
    if indices.dtype != torch.int64:
        raise ValueError(f"iqlhip: update indices must be int64 (got {indices.dtype})")
    if td.dtype != torch.float32:
        raise ValueError(f"iqlhip: TD errors must be float32 (got {td.dtype})")
    if indices.ndim != 1 or td.ndim != 2 or td.shape[1] != 2:
        raise ValueError(f"iqlhip: update indices must be [m] and TD errors [m, 2] (got {tuple(indices.shape)} and "
                         f"{tuple(td.shape)})")
    if indices.shape[0] != td.shape[0]:
        raise ValueError(f"iqlhip: {indices.shape[0]} update indices for {td.shape[0]} rows of TD errors")
    if device is not None and (indices.device != device or td.device != device):
        raise ValueError(f"iqlhip: update indices and TD errors must live on the table's device ({device})")
    return int(indices.shape[0])


def check_priority_args(alpha, eps) -> tuple:
    """(alpha, eps) of the priority (max(|e1|, |e2|) + eps) ** alpha, checked on the host as the library checks them:
    finite floats >= 0, and not both 0 (a zero TD error would give log2(0) * 0).  ValueError otherwise."""
    import math
    out = []
    for name, v in (("alpha", alpha), ("eps", eps)):
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"iqlhip: {name} must be a number, not {type(v).__name__}")
        if not math.isfinite(f) or f < 0.0:
            raise ValueError(f"iqlhip: {name} must be finite and >= 0 (got {v})")
        out.append(f)
    if out[0] == 0.0 and out[1] == 0.0:
        raise ValueError("iqlhip: alpha = 0 needs eps > 0 (a zero TD error would give log2(0) * 0)")
    return out[0], out[1]


def per_member(value, K: int, name: str) -> list:
    """A group call's per-member number: one value for all K members, or a list / tuple / array of K.  Returns K
    entries as given (the caller checks their values); ValueError for another length."""
    if isinstance(value, (list, tuple, np.ndarray)):
        vals = list(value)
        if len(vals) != K:
            raise ValueError(f"iqlhip: {len(vals)} values of {name} for a group of {K}")
        return vals
    return [value] * K


def check_group_priority_args(K: int, alpha, eps) -> tuple:
    """(alphas, epss) of a prioritised group call, each K floats: alpha and eps are one number for all members or K of
    them, every pair checked by check_priority_args (the ValueError names the member)."""
    alphas, epss = per_member(alpha, K, "alpha"), per_member(eps, K, "eps")
    out = []
    for i, (a, e) in enumerate(zip(alphas, epss)):
        try:
            out.append(check_priority_args(a, e))
        except ValueError as err:
            raise ValueError(f"{err} (member {i})") from None
    return [a for a, _ in out], [e for _, e in out]


def check_group_is_beta(K: int, is_beta) -> list:
    """is_beta of a group call as K floats: one number or K of them, each finite and >= 0 (the ValueError names the member)."""
    out = []
    for i, b in enumerate(per_member(is_beta, K, "is_beta")):
        try:
            out.append(check_is_args(1, b, None)[0])
        except ValueError as err:
            raise ValueError(f"{err} (member {i})") from None
    return out


def build_table(w_dev, n: int, stream, updatable: bool = False, capacity=None, max_weight=None, new_row_weight=None):
    """The library's table over the device vector w_dev[0..n): (handle, generation).  new_row_weight not None: an
    updatable table that tracks its maximum."""
    import iqlhip_binding as hb
    table = C.c_void_p()
    if updatable and new_row_weight is not None:
        capacity, max_weight = check_updatable_args(n, capacity, max_weight)
        hb.check(hb.lib().iqlhip_weights_build_tracking(w_dev.data_ptr(), n, capacity, max_weight, float(new_row_weight),
                                                        stream, C.byref(table)))
    elif updatable:
        capacity, max_weight = check_updatable_args(n, capacity, max_weight)
        hb.check(hb.lib().iqlhip_weights_build_updatable(w_dev.data_ptr(), n, capacity, max_weight, stream, C.byref(table)))
    else:
        hb.check(hb.lib().iqlhip_weights_build(w_dev.data_ptr(), n, stream, C.byref(table)))
    gen = C.c_uint64()
    hb.check(hb.lib().iqlhip_weights_info(table, None, None, None, C.byref(gen), None))
    return table, int(gen.value)


def table_state(table, n: int = 0, leaves: bool = False):
    """(total, flags, version, q) of a table, after waiting for the device; q: the n leaf values as a uint64 ndarray
    (leaves=True) or None."""
    import iqlhip_binding as hb
    total, flags, version = C.c_uint64(), C.c_uint32(), C.c_uint64()
    q = np.empty(n, dtype=np.uint64) if leaves else None
    hb.check(hb.lib().iqlhip_weights_state(table, C.byref(total), C.byref(flags), C.byref(version),
                                           q.ctypes.data if leaves else None))
    return int(total.value), int(flags.value), int(version.value), q


def table_max(table) -> tuple:
    """(q_max, w_max) of a tracking table, after waiting for the device."""
    import iqlhip_binding as hb
    q, w = C.c_uint64(), C.c_float()
    hb.check(hb.lib().iqlhip_weights_max(table, C.byref(q), C.byref(w)))
    return int(q.value), float(w.value)


def check_call(buffer) -> int:
    """What every weighted call checks on the buffer before anything is launched: it lives on a GPU, has weights, and
    still draws over the number of rows they were set for (an updatable table spans the buffer's capacity and stays
    valid while the index bound moves: rows beyond it weigh 0).  Returns the number of rows the table weighs."""
    if not getattr(buffer, "_gpu", False):
        raise ValueError("iqlhip: weighted sampling needs a ReplayBuffer that lives on the GPU")
    n = buffer.sample_weights_n
    if n is None:
        raise ValueError("iqlhip: the replay buffer has no sample weights (set_sample_weights)")
    if getattr(buffer, "_weights_updatable", False):
        return n
    if buffer._index_bound() != n:
        raise ValueError(f"iqlhip: the sample weights were set for {n} rows, the buffer now draws over "
                         f"{buffer._index_bound()}: call set_sample_weights again")
    return n


def check_trainer(dp_world: int, dp_exchange, precision: str, batch_size: int, bf16_max_rows: int) -> None:
    """train_steps_weighted's refusals that need no library call: NotImplementedError under data parallelism and for
    bf16 batches beyond the small-batch kernels."""
    if dp_world > 1 or dp_exchange is not None:
        raise NotImplementedError("iqlhip: weighted sampling is not supported under data parallelism")
    if precision == "bf16" and batch_size > bf16_max_rows:
        raise NotImplementedError(f"iqlhip: weighted sampling is not supported for bf16 batches of more than "
                                  f"{bf16_max_rows} rows (got {batch_size}): the large-batch kernels draw uniformly")


class SampleWeights:
    """A weight table of its own: one float32 weight per row position of whatever buffer it is later used with (its
    length must equal that buffer's index bound at the call).  weights: what set_sample_weights takes — a torch tensor
    on a GPU or on the host, or an ndarray — with the same checks and the same ValueErrors; device: where the table
    lives (default: a device tensor's own device, else "cuda"); stream: the raw stream handle the build runs on
    (default: the device's current stream).  The table must stay alive while calls that use it are queued: free() — and
    the destructor — wait for the device first."""
    _table = None
    _n = 0
    _gen = 0
    _device = None
    _updatable = False
    _version = 0
    _tracks = False

    def __init__(self, weights, device=None, stream=None, updatable: bool = False, capacity=None, max_weight=None,
                 track_max: bool = False, new_row_weight=None):
        """updatable=True: a table that update() changes in place.  capacity: rows it spans (default: len(weights));
        rows beyond the given weights weigh 0.  max_weight: fixes the scale for the table's life — weights are
        quantised to multiples of 2^(floor(log2(max(max_weight, max(weights)))) - 38), and a later weight of twice that
        power of two or more saturates; None: the largest weight given.  ValueError for capacity or max_weight without
        updatable=True.  track_max=True (an updatable table only: ValueError otherwise): the table keeps the largest
        priority an applied update or the build has seen — at least new_row_weight (default 1.0, finite and > 0) — and
        insert_max(row) enters a row at it."""
        import torch
        import iqlhip_binding as hb
        shape = tuple(getattr(weights, "shape", ()))
        n = int(shape[0]) if shape else 1        # (n: the vector's own length; check_vector names what else is wrong)
        kind = check_vector(weights, n)
        if not updatable and (capacity is not None or max_weight is not None):
            raise ValueError("iqlhip: capacity and max_weight belong to an updatable table (updatable=True)")
        new_row_weight = check_tracking_args(updatable, track_max, new_row_weight)
        rows = n
        if updatable:
            rows, max_weight = check_updatable_args(n, capacity, max_weight)
        on_gpu = kind == "torch" and weights.device.type != "cpu"
        host = None
        if not on_gpu:                       # (the value checks of a host vector come before any look at a device)
            host = weights if kind == "numpy" else weights.numpy()
            check_host_values(host)
        if device is None:
            dev = weights.device if on_gpu else torch.device("cuda", torch.cuda.current_device())
        else:
            dev = torch.device(device)
            if dev.type != "cuda":
                raise ValueError(f"iqlhip: sample weights live on a GPU, not on {dev}")
            if dev.index is None:
                dev = torch.device("cuda", torch.cuda.current_device())
        if on_gpu:
            if weights.device != dev:
                raise ValueError(f"iqlhip: sample weights live on {weights.device}, the table is asked for on {dev}")
            w_dev = weights.contiguous()
        else:
            w_dev = torch.tensor(host, dtype=torch.float32, device=dev)      # (a copy: the array may be read-only)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
            table, gen = build_table(w_dev, n, st, updatable, rows, max_weight, new_row_weight)
        self._table, self._n, self._gen, self._device = table, rows, gen, dev
        self._updatable, self._version, self._tracks = bool(updatable), 0, bool(track_max)

    @property
    def n(self) -> int:
        """Rows the table weighs (an updatable table: its capacity)."""
        return self._n

    @property
    def updatable(self) -> bool:
        return self._updatable

    @property
    def version(self) -> int:
        """Content version: 0 after the build, plus 1 per update() (a continuation of train_steps_weighted keys on the
        generation and on it)."""
        return self._version

    def _alive(self):
        if self._table is None:
            raise ValueError("iqlhip: the sample weights have been freed")
        return self._table

    def update(self, indices, weights, bound=None) -> None:
        """w[indices[j]] = weights[j] on the device, queued on the current stream, no synchronisation: int64 indices
        and float32 weights, device tensors of one length.  Duplicates: the last position wins.  A NaN, an infinity, a
        negative weight or an index outside [0, bound) (default: the table's n) is skipped and leaves a bit in flags();
        a weight beyond the table's scale saturates.  A draw running on ANOTHER stream at the same time is the caller's
        error.  ValueError on a table that is not updatable."""
        import torch
        import iqlhip_binding as hb
        table = self._alive()
        if not self._updatable:
            raise ValueError("iqlhip: these sample weights are not updatable (SampleWeights(..., updatable=True))")
        m = check_update_args(indices, weights, self._device)
        bound = self._n if bound is None else int(bound)
        if not 0 <= bound <= self._n:
            raise ValueError(f"iqlhip: bound {bound} outside [0, {self._n}]")
        idx, w = indices.contiguous(), weights.contiguous()
        with torch.cuda.device(self._device):
            hb.check(hb.lib().iqlhip_weights_update(table, idx.data_ptr(), w.data_ptr(), m, bound,
                                                    torch.cuda.current_stream(self._device).cuda_stream))
        self._version += 1

    def update_td(self, indices, td, alpha, eps, bound=None) -> None:
        """update() with weights[j] = (max(|td[j, 0]|, |td[j, 1]|) + eps) ** alpha formed on the device inside the update's
        own launches (no torch arithmetic, no intermediate tensor): td is the [m, 2] float32 tensor
        trainer.last_td_errors() returns, indices the rows of that step's batch.  A NaN or an infinity in a TD error is
        skipped and flagged like a non-finite weight.  ValueError for a static table and for alpha or eps negative, not
        finite or both 0."""
        import torch
        import iqlhip_binding as hb
        table = self._alive()
        if not self._updatable:
            raise ValueError("iqlhip: these sample weights are not updatable (SampleWeights(..., updatable=True))")
        m = check_td_args(indices, td, self._device)
        alpha, eps = check_priority_args(alpha, eps)
        bound = self._n if bound is None else int(bound)
        if not 0 <= bound <= self._n:
            raise ValueError(f"iqlhip: bound {bound} outside [0, {self._n}]")
        idx, e = indices.contiguous(), td.contiguous()
        with torch.cuda.device(self._device):
            hb.check(hb.lib().iqlhip_weights_update_td(table, idx.data_ptr(), e.data_ptr(), m, bound, alpha, eps,
                                                       torch.cuda.current_stream(self._device).cuda_stream))
        self._version += 1

    @property
    def tracks_max(self) -> bool:
        """Whether the table tracks its largest priority (track_max=True at the build)."""
        return self._tracks

    def max_priority(self) -> tuple:
        """(q_max, w_max): the largest quantised priority an applied update or the build has seen (never below
        new_row_weight's) and the weight it stands for; waits for the device.  ValueError on a table that does not track."""
        table = self._alive()
        if not self._tracks:
            raise ValueError("iqlhip: these sample weights do not track their maximum (SampleWeights(..., track_max=True))")
        return table_max(table)

    def insert_max(self, row: int, bound=None) -> None:
        """w[row] = the table's largest priority, on the device, queued on the current stream with no synchronisation:
        PER's rule for a newly stored transition.  row in [0, bound), bound (default: n) <= n: ValueError otherwise, and
        on a table that does not track."""
        import torch
        import iqlhip_binding as hb
        table = self._alive()
        if not self._tracks:
            raise ValueError("iqlhip: these sample weights do not track their maximum (SampleWeights(..., track_max=True))")
        row, bound = check_insert_args(row, bound, self._n)
        with torch.cuda.device(self._device):
            hb.check(hb.lib().iqlhip_weights_insert_max(table, row, bound,
                                                        torch.cuda.current_stream(self._device).cuda_stream))
        self._version += 1

    def flags(self) -> int:
        """The sticky flag word (waits for the device): bit 0 a non-finite weight was skipped, bit 1 a negative one,
        bit 2 an index out of range.  0 for a static table."""
        return table_state(self._alive())[1]

    def total(self) -> int:
        """sum(q) as the table holds it now (waits for the device)."""
        return table_state(self._alive())[0]

    def leaves(self) -> np.ndarray:
        """q[0..n) rebuilt from the tree, a uint64 ndarray (waits for the device; tests)."""
        return table_state(self._alive(), self._n, leaves=True)[3]

    def clear_flags(self) -> None:
        import torch
        import iqlhip_binding as hb
        with torch.cuda.device(self._device):
            hb.check(hb.lib().iqlhip_weights_clear_flags(self._alive(), torch.cuda.current_stream(self._device).cuda_stream))

    @property
    def generation(self) -> int:
        """Unique per built table: what a continuation of train_steps_weighted compares."""
        return self._gen

    @property
    def device(self):
        return self._device

    def free(self) -> None:
        """Wait for the device, then free the table; the object refuses every later use."""
        table, self._table = self._table, None
        if table is not None:
            import iqlhip_binding as hb
            hb.lib().iqlhip_weights_free(table)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def draw_indices(self, n: int, seed: int, offset: int, is_beta=None, batch_size=None):
        """Indices 0 .. n - 1 of the weighted index stream (seed, offset) as a device int64 tensor
        (ReplayBuffer.draw_weighted_indices for this table).  With is_beta: (idx, c), see draw_with_is."""
        import torch
        import iqlhip_binding as hb
        if self._table is None:
            raise ValueError("iqlhip: the sample weights have been freed")
        if n < 1:
            raise ValueError("iqlhip: n must be at least 1")
        if is_beta is not None:
            return draw_with_is(self._table, self._device, n, seed, offset, is_beta, batch_size,
                                torch.cuda.current_stream(self._device).cuda_stream)
        if batch_size is not None:
            raise ValueError("iqlhip: batch_size only means something together with is_beta")
        idx = torch.empty(int(n), dtype=torch.int64, device=self._device)
        with torch.cuda.device(self._device):
            hb.check(hb.lib().iqlhip_draw_indices_weighted(idx.data_ptr(), int(n), self._table,
                                                           int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF,
                                                           torch.cuda.current_stream(self._device).cuda_stream))
        return idx


def check_is_args(n: int, is_beta, batch_size) -> tuple:
    """(is_beta, batch_size) of a draw with importance-sampling weights, checked on the host: is_beta a finite float
    >= 0, batch_size (default: all n indices are one batch) an integer in [1, n]."""
    import math
    try:
        beta = float(is_beta)
    except (TypeError, ValueError):
        raise ValueError(f"iqlhip: is_beta must be a number, not {type(is_beta).__name__}")
    if not math.isfinite(beta) or beta < 0.0:
        raise ValueError(f"iqlhip: is_beta must be finite and >= 0 (got {is_beta})")
    bs = int(n) if batch_size is None else int(batch_size)
    if bs < 1 or bs > int(n):
        raise ValueError(f"iqlhip: batch_size {batch_size} outside [1, n={n}]")
    return beta, bs


def draw_with_is(table, device, n: int, seed: int, offset: int, is_beta, batch_size, stream):
    """(idx, c): the indices of the weighted stream and the importance-sampling weights of the drawn rows,
    c = (q_min / q_row) ** is_beta with q_min the smallest quantised weight among the batch_size consecutive indices of the
    row's batch — float32 on the device, in (0, 1], what trainer.train(batch, loss_weights=c) takes."""
    import torch
    import iqlhip_binding as hb
    beta, bs = check_is_args(n, is_beta, batch_size)
    idx = torch.empty(int(n), dtype=torch.int64, device=device)
    c = torch.empty(int(n), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        hb.check(hb.lib().iqlhip_draw_indices_weighted_is(idx.data_ptr(), c.data_ptr(), int(n), table,
                                                          int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF,
                                                          bs, beta, stream))
    return idx, c


def check_table(buffer, weights, member=None) -> int:
    """A SampleWeights used with `buffer` instead of the buffer's own table: the buffer lives on a GPU, the table is
    alive, on the buffer's device, and weighs exactly the rows the buffer draws over.  Returns that number."""
    who = "" if member is None else f" (member {member})"
    if not isinstance(weights, SampleWeights):
        raise ValueError(f"iqlhip: weights must be a SampleWeights, not {type(weights).__name__}{who}")
    if not getattr(buffer, "_gpu", False):
        raise ValueError(f"iqlhip: weighted sampling needs a ReplayBuffer that lives on the GPU{who}")
    if weights._table is None:
        raise ValueError(f"iqlhip: the sample weights have been freed{who}")
    rows = getattr(buffer, "_rows", None)
    if rows is not None and weights.device is not None and rows.device != weights.device:
        raise ValueError(f"iqlhip: the sample weights live on {weights.device}, the buffer on {rows.device}{who}")
    n = buffer._index_bound()
    if weights.updatable:           # (spans a capacity: rows beyond the index bound weigh 0 unless the caller set them)
        if not n <= weights.n <= buffer._buffer_size:
            raise ValueError(f"iqlhip: the updatable sample weights span {weights.n} rows, the buffer draws over {n} of "
                             f"{buffer._buffer_size}{who}")
        return weights.n
    if weights.n != n:
        raise ValueError(f"iqlhip: the sample weights cover {weights.n} rows, the buffer draws over {n}{who}")
    return n


def check_group_call(buffers, weights, K: int):
    """Which table each of a group's K members draws by, checked before anything is launched.  buffers: K buffers, or
    one shared by all members.  weights: None — every member uses its buffer's own table (check_call: ValueError for a
    buffer without one); one SampleWeights — all members use it; a list of K entries, each a SampleWeights or None —
    a None member draws uniformly.  Lengths are checked against each member's buffer's index bound.  Returns K
    entries: the member's buffer (its own table), a SampleWeights, or None (uniform)."""
    bufs = list(buffers) if isinstance(buffers, (list, tuple)) else [buffers] * K
    if len(bufs) != K:
        raise ValueError(f"iqlhip: a group of {K} needs {K} buffers (or one shared buffer), got {len(bufs)}")
    if weights is None:
        for i, b in enumerate(bufs):
            try:
                check_call(b)
            except ValueError as e:
                raise ValueError(f"{e} (member {i})") from None
        return list(bufs)
    if isinstance(weights, SampleWeights):
        entries = [weights] * K
    elif isinstance(weights, (list, tuple)):
        entries = list(weights)
        if len(entries) != K:
            raise ValueError(f"iqlhip: {len(entries)} weight tables for a group of {K}")
    else:
        raise ValueError("iqlhip: weights must be None, a SampleWeights, or a list with a SampleWeights or None per "
                         f"member, not {type(weights).__name__}")
    for i, (b, w) in enumerate(zip(bufs, entries)):
        if w is None:
            if not getattr(b, "_gpu", False):
                raise ValueError(f"iqlhip: train_steps needs a ReplayBuffer that lives on the GPU (member {i})")
            continue
        check_table(b, w, i)
    return entries


def check_group_prioritized(buffers, weights, K: int):
    """check_group_call for a prioritised group call, which updates every member's table: each of the K members needs an
    UPDATABLE table (no None entry), and no two members the same one — their updates would race, and "where the solo call
    leaves the member" would mean nothing.  Sharing a buffer's rows is fine; its own table can then serve one member only.
    Returns the K entries (a buffer — its own table — or a SampleWeights).  ValueError otherwise, before any library call."""
    entries = check_group_call(buffers, weights, K)
    for i, e in enumerate(entries):
        if e is None:
            raise ValueError(f"iqlhip: prioritised replay needs a table for every member (member {i} has none)")
        updatable = e.updatable if isinstance(e, SampleWeights) else getattr(e, "_weights_updatable", False)
        if not updatable:
            raise ValueError("iqlhip: prioritised replay needs updatable sample weights "
                             f"(set_sample_weights(..., updatable=True) / SampleWeights(..., updatable=True); member {i})")
        tracks = e.tracks_max if isinstance(e, SampleWeights) else getattr(e, "_weights_tracks", False)
        if tracks:
            raise NotImplementedError("iqlhip: sample weights that track their maximum (track_max=True) are not supported "
                                      f"in trainer groups (member {i})")
        for j in range(i):
            if entries[j] is e:
                raise ValueError(f"iqlhip: member {i} draws by the table of member {j}: a prioritised call updates one "
                                 "table per member (give each member a SampleWeights of its own)")
    return entries
