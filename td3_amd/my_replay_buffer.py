"""HBM-resident replay buffers with the reference's Python surface.

Drop-in for ``/root/reference/my_replay_buffer.py``:

* ``ReplayBuffer_featured(obs_space, action_space, max_size=1e6, load_folder=None)``
  (:72-89) with ``add`` (:109-117), ``sample`` (:119-128), ``save`` / ``load``
  (:91-107) and the ``ptr`` / ``size`` / ``max_size`` attributes.
* ``ReplayBuffer_particles`` (:6-69), the same over (features, particles) states.

The storage lives in HBM (``libtd3hip``'s ring, one fp32 record per transition).
``add`` writes the transition straight into a host array of ring records (the fp32
cast the reference makes at ``sample``, :122-127, made once at ``add``: the same
rounding of the same float64 values) and ``flush`` ships the staged records in one
``rb_add_records`` call; ``sample`` / ``TD3.train`` flush first, so a transition
added at step t is samplable at step t exactly as in the reference (main.py:261
before :269).
``sample`` draws indices with a device Philox stream instead of the global numpy
MT19937 (``np.random.randint`` at :120) -- a documented, deliberate difference.

``host_shadow=True`` also keeps the reference's own float64 host arrays (:79-85 / :15-22) of
every row ``add`` / ``add_batch`` / ``load`` received, written by the same numpy row
assignments; ``save`` then writes those, so a reference folder loaded and saved back, or a
run resumed from a build-saved folder, sees the bytes the reference wrote.  Without it ``save``
writes the fp32 ring (float64(float32(x))).  The fp32 ring stays the training copy either way.
"""
from __future__ import annotations

import math
import os
import pickle

import numpy as np

from . import _lib
from ._lib import check

_STAGE_ROWS = 4096


def _torch():
    import torch
    return torch


def default_device_index() -> int:
    torch = _torch()
    if not torch.cuda.is_available():
        raise RuntimeError("td3_amd needs a ROCm GPU (torch.cuda.is_available() is False)")
    if "LOCAL_RANK" in os.environ:
        return int(os.environ["LOCAL_RANK"]) % torch.cuda.device_count()
    return torch.cuda.current_device()


def _is_cuda_tensor(x) -> bool:
    """A torch tensor on a GPU (without importing torch for numpy callers)."""
    return bool(getattr(x, "is_cuda", False))


def _device_rows(dev, arrays, widths, what):
    """The inputs of a device add as contiguous fp32 tensors on ``dev`` (``[n][w]``, ``[n]`` where
    the width is 0) and their common row count n; a ValueError naming ``what`` when the counts differ."""
    torch = _torch()
    ts = []
    for x, w in zip(arrays, widths):
        x = torch.as_tensor(x, device=dev).to(torch.float32)
        ts.append(x.reshape(-1, w).contiguous() if w else x.reshape(-1).contiguous())
    n = ts[0].shape[0]
    if any(t.shape[0] != n for t in ts):
        raise ValueError(f"{what} must have the same number of rows")
    return ts, n


def _hindsight_device(dev, goal_cols, goals, rewards, n):
    """The ``rb_hindsight`` of a device add of n transitions and the fp32 tensors it points to."""
    torch = _torch()
    g = torch.as_tensor(goals, device=dev).to(torch.float32).contiguous()
    r = torch.as_tensor(rewards, device=dev).to(torch.float32).contiguous()
    cols, K, G = _hindsight_dims(goal_cols, g, r, n)
    hs = _lib.rb_hindsight()
    hs.k, hs.g = K, G
    for j, c in enumerate(cols):
        hs.cols[j] = c
    hs.goals, hs.rewards = g.data_ptr(), r.data_ptr()
    return hs, (g, r)


def _hindsight_dims(goal_cols, goals, rewards, n):
    """``(cols, K, G)`` of the relabels of n transitions: ``rewards`` is ``[n][K]``, ``goals``
    ``[n][K][G]`` (or ``[n][K]`` when there is one goal column); anything else is a ValueError."""
    cols = [int(c) for c in (goal_cols.tolist() if hasattr(goal_cols, "tolist") else goal_cols)]
    G = len(cols)
    if not 1 <= G <= 8:
        raise ValueError(f"add_batch_hindsight: goal_cols must name 1..8 columns, got {G}")
    rs, gs = tuple(rewards.shape), tuple(goals.shape)
    if len(rs) != 2 or rs[0] != n:
        raise ValueError(f"add_batch_hindsight: rewards must be [n][K] with n = {n}, got {rs}")
    K = rs[1]
    if gs != (n, K, G) and not (G == 1 and gs == (n, K)):
        raise ValueError(f"add_batch_hindsight: goals must be [n][K][G] = {(n, K, G)}, got {gs}")
    return cols, K, G


def _hindsight_expand(arrs, state_slots, reward_slot, cols, K, goals, rewards):
    """The n * (1 + K) expanded float64 rows of main.py:70-91 from n source rows: row i * (1 + K) is
    transition i, rows i * (1 + K) + j (j = 1..K) its relabels (goals[i][j - 1] in columns ``cols``
    of the arrays ``state_slots``, rewards[i][j - 1] in array ``reward_slot``)."""
    n, width = arrs[state_slots[0]].shape
    if len(set(cols)) != len(cols) or not all(0 <= c < width for c in cols):
        raise ValueError(f"add_batch_hindsight: goal_cols must be distinct columns in [0, {width}), got {cols}")
    out = [np.repeat(a, 1 + K, axis=0) for a in arrs]
    g = np.asarray(goals, dtype=np.float64).reshape(n, K, len(cols))
    for k in state_slots:
        out[k].reshape(n, 1 + K, -1)[:, 1:, cols] = g
    out[reward_slot].reshape(n, 1 + K)[:, 1:] = np.asarray(rewards, dtype=np.float64).reshape(n, K)
    return out


class _SafeIntUnpickler(pickle.Unpickler):
    """ptr.pkl / size.pkl hold a pickled int (my_replay_buffer.py:93-95); refuse anything else."""

    def find_class(self, module, name):
        raise pickle.UnpicklingError(f"refusing to load {module}.{name} from a buffer file")


class _TorchOrder:
    """Orders work on one of the library's non-blocking streams against torch's current stream:
    on entry the library stream waits for torch's (tensors it reads or fills were made there),
    on exit torch's stream waits for the library's (its outputs are then safe to use)."""

    def __init__(self, stream_ptr, device):
        torch = _torch()
        self._torch_s = torch.cuda.current_stream(device)
        self._lib_s = torch.cuda.ExternalStream(int(stream_ptr), device=device)

    def __enter__(self):
        self._lib_s.wait_stream(self._torch_s)
        return self._lib_s

    def __exit__(self, *exc):
        self._torch_s.wait_stream(self._lib_s)
        return False


class _HostShadow:
    """The reference's float64 arrays (``store_np`` order, the reference's shapes), written row
    by row in ring order with the reference's own assignments (my_replay_buffer.py:109-117)."""

    def __init__(self, arrays, ptr=0):
        self.arrays = arrays                       # name -> ndarray, first dim = capacity
        self.cap = next(iter(arrays.values())).shape[0]
        self.ptr = int(ptr) % self.cap
        self.valid = True                          # False once a device-only write happened

    @classmethod
    def zeros(cls, shapes):
        return cls({k: np.zeros(shp) for k, shp in shapes.items()})

    def put(self, values):
        """One transition: ``values`` in store_np order (not_done already 1 - done)."""
        for arr, v in zip(self.arrays.values(), values):
            arr[self.ptr] = v
        self.ptr = (self.ptr + 1) % self.cap

    def put_batch(self, values, n):
        """n transitions (arrays of n rows each), as n consecutive ``put``."""
        skip = max(0, n - self.cap)                # rows a later row of the batch overwrites
        rows = (self.ptr + skip + np.arange(n - skip)) % self.cap
        for arr, v in zip(self.arrays.values(), values):
            arr[rows] = np.asarray(v).reshape((n,) + arr.shape[1:])[skip:]
        self.ptr = (self.ptr + n) % self.cap


def _save_folder(folder, ptr, size, arrays):
    """my_replay_buffer.py:91-99 / :24-32: ptr / size pickled (protocol 4), arrays np.save'd."""
    os.makedirs(folder, exist_ok=True)
    for attrib, v in (("ptr", int(ptr)), ("size", int(size))):
        with open(os.path.join(folder, attrib + ".pkl"), "wb") as f:
            pickle.dump(v, f, protocol=4)
    for attrib, arr in arrays.items():
        with open(os.path.join(folder, attrib + ".pkl"), "wb") as f:
            np.save(f, arr)


def _load_int(path):
    with open(path, "rb") as f:
        v = _SafeIntUnpickler(f).load()
    if not isinstance(v, (int, np.integer)):
        raise ValueError(f"{path}: expected an int, got {type(v)}")
    return int(v)


class _RingBuffer(object):
    """What the two ring kinds share: the handle, the records staged by ``add``, the batch adds,
    ``sample`` and ``save`` / ``load``.  All of it walks one field table, ``_fields``, built in
    ``_create``: per ``store_np`` array its name, flat width and per-row shape, in record order
    (replay.h: the fields lie one behind the other from column 0; the last one is not_done).

    A kind supplies ``store_np``, its reading of ``obs_space``, ``_dims`` / ``_row_shapes`` /
    ``_dims_from``, the names of its C calls (``_C``), how its inputs are counted in messages
    (``_count``), the fields hindsight relabels (``_relabel``: the two states, the reward), the length
    of its stage and the public ``add`` / ``add_batch`` / ``add_batch_hindsight`` signatures."""

    store_pkl = ["ptr", "size"]

    def __init__(self, obs_space, action_space, max_size=int(1e6), load_folder=None,
                 device=None, seed=0, host_shadow=False):
        self._lib = _lib.load()
        self.host_shadow = bool(host_shadow)
        self._shadow = None
        self._read_spaces(obs_space, action_space)
        self._dev = default_device_index() if device is None else int(device)
        torch = _torch()
        self.device = torch.device("cuda", self._dev)
        self.seed = int(seed)
        self._h = None
        self._n = 0
        self._per = None                         # (alpha, eps) once enable_priorities was called
        if load_folder is not None:
            self.load(load_folder)
        else:
            self._create(int(max_size))

    # ------------------------------------------------------------------ plumbing
    def _call(self, name, *args):
        check(getattr(self._lib, name)(*args), name)

    def _create(self, max_size):
        import ctypes as C
        if self._h is not None:
            self._lib.rb_destroy(self._h)
            self._h = None
        h = C.c_void_p()
        self._call(self._C["create"], *self._dims(), max_size, self._dev, self.seed, C.byref(h))
        self._h = h
        self.max_size = max_size
        self.record_floats = self._info().record_floats
        self._fields = tuple((name, int(np.prod(shape)), tuple(shape))
                             for name, shape in zip(self.store_np, self._row_shapes()))
        widths = [w for _, w, _ in self._fields]
        assert self.record_floats == (sum(widths) + 3) // 4 * 4, "field table out of step with rb_info"
        self._cols = tuple(slice(sum(widths[:k]), sum(widths[:k + 1])) for k in range(len(widths)))
        self._widths = tuple(widths[:-2]) + (0, 0)   # of the add inputs: reward and done are [n]
        # host records staged by ``add`` (zeroed: the record pad stays 0) and their float*
        self._stage = np.zeros((self._stage_rows, self.record_floats), dtype=np.float32)
        self._stage_ptr = _lib.fptr(self._stage)
        self._n = 0
        self._shadow = _HostShadow.zeros(self._shapes(max_size)) if self.host_shadow else None
        if self._per is not None:                # a ring re-created by load() keeps its priorities on
            self._call("rb_enable_priorities", self._h, *self._per, self._stream())

    def _shapes(self, n):
        return {name: (n, *shape) for name, _, shape in self._fields}

    def _info(self):
        info = _lib.rb_info_t()
        check(self._lib.rb_info(self._h, info), "rb_info")
        return info

    @property
    def handle(self):
        return self._h

    @property
    def ptr(self):
        self.flush()
        return int(self._info().ptr)

    @property
    def size(self):
        self.flush()
        return int(self._info().size)

    def _stream(self):
        return None                      # the ring's own stream (see _torch_order)

    def _torch_order(self):
        return _TorchOrder(self._lib.rb_stream(self._h), self.device)

    def flush(self, stream=None):
        """Ship the staged records; ``stream`` (a learner's, from ``TD3.train``) queues them in that
        stream's order, so the step that samples them needs no cross-stream event (replay.h)."""
        n = self._n
        if n:
            self._n = 0
            check(self._lib.rb_add_records(self._h, self._stage_ptr, n, stream), "rb_add_records")

    # ------------------------------------------------------------------ batch adds
    def _add_batch(self, *arrays):
        self.flush()
        if _is_cuda_tensor(arrays[0]):
            self._add_batch_device(*arrays)
            return
        first = np.ascontiguousarray(arrays[0], dtype=np.float64).reshape(-1, self._widths[0])
        n = first.shape[0]
        arrs = [first] + [np.ascontiguousarray(x, dtype=np.float64).reshape((n, w) if w else (n,))
                          for x, w in zip(arrays[1:], self._widths[1:])]
        if self._shadow is not None:
            self._shadow.put_batch(arrs[:-1] + [1. - arrs[-1]], n)
        self._call(self._C["add"], self._h, *[_lib.dptr(x) for x in arrs], n, self._stream())

    def _add_batch_device(self, *arrays):
        ts, n = _device_rows(self.device, arrays, self._widths, f"add_batch: the {self._count} inputs")
        if self._shadow is not None:
            self._shadow.valid = False           # rows the host never saw: save() writes the ring
        # the tensors were made on torch's stream; on exit torch's stream waits for the ring's, so
        # the blocks freed with them are reused only after the add read them
        with self._torch_order():
            self._call(self._C["add_device"], self._h, *[t.data_ptr() for t in ts], n, self._stream())

    def _add_batch_hindsight(self, arrays, goal_cols, goals, rewards):
        self.flush()
        what = f"add_batch_hindsight: the {self._count} inputs"
        if _is_cuda_tensor(arrays[0]):
            ts, n = _device_rows(self.device, arrays, self._widths, what)
            hs, keep = _hindsight_device(self.device, goal_cols, goals, rewards, n)
            if n == 0:
                return
            if self._shadow is not None:
                self._shadow.valid = False       # rows the host never saw: save() writes the ring
            with self._torch_order():            # as _add_batch_device; `keep` lives until the exit
                self._call(self._C["add_device_hindsight"], self._h, *[t.data_ptr() for t in ts], n, hs,
                           self._stream())
            return
        arrs = [np.ascontiguousarray(arrays[0], dtype=np.float64).reshape(-1, self._widths[0])]
        arrs += [np.asarray(x, dtype=np.float64).reshape((-1, w) if w else (-1,))
                 for x, w in zip(arrays[1:], self._widths[1:])]
        n = arrs[0].shape[0]
        if any(x.shape[0] != n for x in arrs):
            raise ValueError(f"{what} must have the same number of rows")
        goals, rewards = np.asarray(goals), np.asarray(rewards)
        cols, K, _ = _hindsight_dims(goal_cols, goals, rewards, n)
        if n:
            self.add_batch(*_hindsight_expand(arrs, *self._relabel, cols, K, goals, rewards))

    def _add_batch_nstep(self, arrays, ended, n, gamma):
        self.flush()
        if not all(_is_cuda_tensor(x) for x in (*arrays, ended)):
            raise TypeError("add_batch_nstep takes CUDA tensors only: the stored rows mature in the ring "
                            "on the device, there is no host path")
        torch = _torch()
        ts, rows = _device_rows(self.device, arrays, self._widths, f"add_batch_nstep: the {self._count} inputs")
        if ended.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"add_batch_nstep: ended must be a bool or uint8 tensor, got {ended.dtype}")
        e = ended.to(self.device).reshape(-1).contiguous().view(torch.uint8)
        if e.shape[0] != rows:
            raise ValueError(f"add_batch_nstep: ended must have one entry per row ({rows}), got {e.shape[0]}")
        if rows == 0:                            # an empty tensor has no address; the checks still run
            e = torch.zeros(1, dtype=torch.uint8, device=self.device)
        ns = _lib.rb_nstep()
        ns.n, ns.gamma, ns.ended = int(n), float(gamma), e.data_ptr()
        with self._torch_order():                # as _add_batch_device; `e` lives until the exit
            self._call(self._C["add_device_nstep"], self._h, *[t.data_ptr() for t in ts], rows, ns, self._stream())
        if rows and self._shadow is not None:
            self._shadow.valid = False           # rows the host never saw: save() writes the ring

    def fill_synthetic(self, n, max_action=1.0, seed=0):
        """Device-side prefill with the SURVEY §8(d) synthetic distribution (bench/tests)."""
        self.flush()
        if self._shadow is not None:
            self._shadow.valid = False           # rows the host never saw: save() writes the ring
        check(self._lib.rb_fill_synthetic(self._h, int(n), float(max_action), int(seed),
                                          self._stream()), "rb_fill_synthetic")

    def sample(self, batch_size, indices=None, return_indices=False):
        """my_replay_buffer.py:119-128 / :58-69: the ``store_np`` fields of the drawn rows, fp32 on
        the device (5 tensors, or 7 with the particle blocks as ``[B][N][D]``)."""
        torch = _torch()
        self.flush()
        B = int(batch_size)
        dev = self.device
        out = tuple(torch.empty((B, *shape), device=dev, dtype=torch.float32) for _, _, shape in self._fields)
        idx_out = torch.empty((B,), device=dev, dtype=torch.int64)
        inj = None
        if indices is not None:
            inj = torch.as_tensor(np.asarray(indices, dtype=np.int64), device=dev)
            if inj.numel() != B:
                raise ValueError("indices must have batch_size entries")
            size = self.size
            if B and (int(inj.min()) < 0 or int(inj.max()) >= max(size, 1)):
                raise IndexError("index out of range of the filled buffer")
        with self._torch_order():
            self._call(self._C["sample"], self._h, B, *[t.data_ptr() for t in out],
                       inj.data_ptr() if inj is not None else None, idx_out.data_ptr(), self._stream())
        if return_indices:
            return out, idx_out
        return out

    # ------------------------------------------------------------------ dataset normalisation
    def _call_on_torch_stream(self, name, *args):
        """A ring call in the order of torch's current stream: on that stream itself, or -- torch's
        default stream is the null stream, which the C call reads as "the ring's own" -- on the ring's
        stream between two waits (``_torch_order``), so the statistics' ticks on torch's stream and this
        call see each other's results either way."""
        stream = _torch().cuda.current_stream(self.device).cuda_stream
        if stream:
            self._call(name, *args, stream)
        else:
            with self._torch_order():
                self._call(name, *args, None)

    def state_moments(self, stats=None, *, merge=False, gamma=0.99, obs_clip=10.0, eps=1e-8, col_mask=None):
        """The moments of the stored states (``state``; ``state_features`` of a particle ring) over the
        rows ``[0, size)`` into the observation moments of ``stats`` (``rb_state_moments``: on the device,
        on torch's current stream, nothing read back) -- what TD3+BC normalises a dataset with.  Without
        ``stats`` a ``RolloutStats(1, state width)`` is made on the ring's device from ``gamma`` /
        ``obs_clip`` / ``eps`` / ``col_mask``.  ``merge`` adds the ring's rows to the moments ``stats``
        already holds (Chan's merge) instead of replacing them.  Returns ``stats``: hand
        ``stats.frozen_copy(n_envs)`` to ``NormalizedVecEnv(..., update=False)`` for the online rows."""
        from .rollout_stats import RolloutStats
        self.flush()
        if stats is None:
            stats = RolloutStats(1, self._dims()[0], gamma=gamma, obs_clip=obs_clip, eps=eps, col_mask=col_mask,
                                 device=self._dev)
        self._call_on_torch_stream("rb_state_moments", self._h, stats._h, 1 if merge else 0)
        return stats

    def normalize_states(self, stats):
        """Normalise the stored states and next states of the rows ``[0, size)`` in place with the
        moments of ``stats`` (``rb_normalize_states``: ``rs_tick``'s own element expression, so these rows
        and the rows a ``NormalizedVecEnv`` on the same frozen moments stores agree bit for bit).  Once
        per ring: ``normalized`` is then set, until ``load`` / ``fill_synthetic`` bring raw rows again."""
        self.flush()
        self._call_on_torch_stream("rb_normalize_states", self._h, stats._h)
        if self._shadow is not None:
            self._shadow.valid = False           # rows the host never saw: save() writes the ring

    @property
    def normalized(self):
        info = _lib.rb_norm_info_t()
        check(self._lib.rb_norm_info(self._h, info), "rb_norm_info")
        return bool(info.normalized)

    # ------------------------------------------------------------------ priorities
    def enable_priorities(self, alpha=0.6, eps=1e-6):
        """Prioritized replay (Schaul et al. 2016): per-row priorities in a sum tree next to the ring
        (``rb_enable_priorities``).  The rows already stored get priority 1, every row added later the
        largest priority stored so far; ``TD3.train`` then draws rows in proportion to their
        priorities, weights the critic loss and writes ``(|TD error| + eps) ** alpha`` back.  The
        arguments are remembered: ``load()`` re-creates the ring and enables them again (all loaded
        rows then have one priority; ``save()`` does not store priorities)."""
        self.flush()
        self._call("rb_enable_priorities", self._h, float(alpha), float(eps), self._stream())
        self._per = (float(alpha), float(eps))

    @property
    def prioritized(self):
        return self._per is not None

    def sample_prioritized(self, batch_size, beta, u=None):
        """``(idx, weights)``: int64 rows drawn in proportion to their priorities (stratified: draw k
        from the k-th of ``batch_size`` equal slices of the total mass) and their importance weights
        ``(size * p / total) ** -beta``, normalised by the largest of the batch; CUDA tensors.  ``u``
        (``[batch_size]`` mass fractions in [0, 1)) replaces the Philox draw."""
        torch = _torch()
        self.flush()
        B = int(batch_size)
        idx = torch.empty((B,), device=self.device, dtype=torch.int64)
        w = torch.empty((B,), device=self.device, dtype=torch.float32)
        inj = None
        if u is not None:
            inj = torch.as_tensor(u, device=self.device).to(torch.float32).reshape(-1).contiguous()
            if inj.numel() != B:
                raise ValueError("u must have batch_size entries")
        with self._torch_order():
            self._call("rb_sample_prioritized", self._h, B, float(beta),
                       inj.data_ptr() if inj is not None else None, idx.data_ptr(), w.data_ptr(), self._stream())
        return idx, w

    def _store_priorities(self, call, idx, values):
        torch = _torch()
        self.flush()
        if not (_is_cuda_tensor(idx) and _is_cuda_tensor(values)):
            raise TypeError(f"{call} takes CUDA tensors (indices and values stay on the device)")
        i = idx.to(self.device, torch.int64).reshape(-1).contiguous()
        v = values.to(self.device, torch.float32).reshape(-1).contiguous()
        if i.numel() != v.numel():
            raise ValueError(f"{call}: idx and values must have the same number of entries")
        if i.numel() == 0:                       # an empty tensor has no address
            self._call(call, self._h, None, None, 0, self._stream())
            return
        with self._torch_order():                # as _add_batch_device: i and v live until the exit
            self._call(call, self._h, i.data_ptr(), v.data_ptr(), i.numel(), self._stream())

    def update_priorities(self, idx, td_abs):
        """Priorities of rows ``idx`` = ``(td_abs + eps) ** alpha`` (CUDA tensors; ``rb_update_priorities``)."""
        self._store_priorities("rb_update_priorities", idx, td_abs)

    def set_priorities(self, idx, p):
        """Priorities of rows ``idx`` = ``p`` as given, finite and >= 0 (CUDA tensors); 0 takes a row
        out of the draw."""
        self._store_priorities("rb_set_priorities", idx, p)

    def priorities(self):
        """The priority of every ring row, numpy ``[max_size]`` (0 for rows never written)."""
        self.flush()
        out = np.empty((self.max_size,), dtype=np.float32)
        check(self._lib.rb_get_priorities(self._h, 0, self.max_size, _lib.fptr(out)), "rb_get_priorities")
        return out

    def priority_info(self):
        """``dict`` of enabled, alpha, eps, levels (of the tree), total (the sum of all priorities as
        the draw sees it) and max_priority (what a new row receives)."""
        self.flush()
        info = _lib.rb_priority_info_t()
        check(self._lib.rb_priority_info(self._h, info), "rb_priority_info")
        return {k: getattr(info, k) for k, _ in info._fields_}

    # ------------------------------------------------------------------ persistence
    def _records(self):
        n = self.max_size
        rec = np.empty((n, self.record_floats), dtype=np.float32)
        check(self._lib.rb_read_records(self._h, 0, n, _lib.fptr(rec)), "rb_read_records")
        return rec

    def save(self, folder):
        """my_replay_buffer.py:91-99 / :24-32: ptr/size pickled (protocol 4), arrays via np.save (the
        float64 host shadow when kept, else the fp32 ring widened)."""
        self.flush()
        info = self._info()
        sh = self._shadow
        if sh is not None and sh.valid:
            assert sh.ptr == int(info.ptr) % sh.cap, "host shadow out of step with the ring"
            arrays = sh.arrays
        else:
            rec = self._records()
            arrays = {name: rec[:, c].astype(np.float64).reshape((self.max_size, *shape))
                      for (name, _, shape), c in zip(self._fields, self._cols)}
        _save_folder(folder, info.ptr, info.size, arrays)

    def load(self, folder):
        """my_replay_buffer.py:101-107 / :34-44 (pickles are read by an int-only unpickler)."""
        self._n = 0                         # rows added before a load are replaced with it
        ptr = _load_int(os.path.join(folder, "ptr.pkl"))
        size = _load_int(os.path.join(folder, "size.pkl"))
        arrs = {}
        for attrib in self.store_np:
            with open(os.path.join(folder, attrib + ".pkl"), "rb") as f:
                arrs[attrib] = np.load(f, allow_pickle=False)
        n = arrs[self.store_np[0]].shape[0]
        self._dims_from(arrs)
        self._create(n)
        if self.host_shadow:                     # the loaded arrays themselves, bytes untouched
            self._shadow = _HostShadow(arrs, ptr)
        rec = np.zeros((n, self.record_floats), dtype=np.float32)
        for (name, w, _), c in zip(self._fields, self._cols):
            rec[:, c] = arrs[name].reshape(n, w)
        check(self._lib.rb_write_records(self._h, 0, n, _lib.fptr(rec), ptr % n, min(size, n)),
              "rb_write_records")

    def __del__(self):
        try:
            if self._h is not None and _lib.alive():
                self._lib.rb_destroy(self._h)
                self._h = None
        except Exception:
            pass


class ReplayBuffer_featured(_RingBuffer):
    """Flat-observation replay ring (my_replay_buffer.py:72-128) resident in HBM."""

    store_np = ["state", "action", "next_state", "reward", "not_done"]
    _C = {"create": "rb_create", "add": "rb_add", "add_device": "rb_add_device",
          "add_device_hindsight": "rb_add_device_hindsight", "add_device_nstep": "rb_add_device_nstep",
          "sample": "rb_sample"}
    _count = "five"
    _relabel = ((0, 2), 3)
    _stage_rows = _STAGE_ROWS

    def _read_spaces(self, obs_space, action_space):
        self.state_dim = int(obs_space.shape[0])
        self.action_dim = int(action_space.shape[0])

    def _dims(self):
        return self.state_dim, self.action_dim

    def _row_shapes(self):
        sd, ad = self._dims()
        return (sd,), (ad,), (sd,), (1,), (1,)

    def _dims_from(self, arrs):
        self.state_dim = arrs["state"].shape[1]
        self.action_dim = arrs["action"].shape[1]

    def add(self, state, action, next_state, reward, done):
        """my_replay_buffer.py:109-117 (stores not_done = 1 - done): numpy row assignment as the
        reference's, into the staged fp32 record."""
        row = self._stage[self._n]
        cs, ca, cs2, cr, cnd = self._cols
        row[cs] = state
        row[ca] = action
        row[cs2] = next_state
        row[cr] = reward
        row[cnd] = 1. - np.asarray(done, dtype=np.float64)
        if self._shadow is not None:
            self._shadow.put((state, action, next_state, reward, 1. - done))
        self._n += 1
        if self._n == len(self._stage):
            self.flush()

    def add_batch(self, state, action, next_state, reward, done):
        """Bulk add of n transitions (experience_injection.py / hindsight relabel path).  Torch
        CUDA tensors (a GPU-resident environment's rows, any float dtype) go from device memory
        straight into the ring (``rb_add_device``): no host copy, no synchronisation."""
        self._add_batch(state, action, next_state, reward, done)

    def add_batch_hindsight(self, state, action, next_state, reward, done, *, goal_cols, goals, rewards):
        """``add_to_replay_buffer`` with K hindsight relabels per transition (main.py:70-91) for n
        transitions at once: the ring receives, for each transition in turn, the transition and then
        its K relabels -- the same row with ``goals[i][j]`` (``[n][K][G]``, or ``[n][K]`` when
        ``goal_cols`` names one column) in columns ``goal_cols`` of state and next_state and
        ``rewards[i][j]`` (``[n][K]``) as the reward.  Exactly ``add_batch`` of those n * (1 + K)
        rows.  CUDA tensors are fanned out by the add kernel itself (``rb_add_device_hindsight``:
        no expanded copy is made); host arrays are expanded in float64 and take the host add."""
        self._add_batch_hindsight((state, action, next_state, reward, done), goal_cols, goals, rewards)

    def add_batch_nstep(self, state, action, next_state, reward, done, *, ended, n, gamma):
        """One tick of a vectorised device rollout with n-step returns (``rb_add_device_nstep``): row i is
        environment i at every call.  The tick's rows are stored as ``add_batch`` stores them and, in
        the same launch, the rows the previous ``n - 1`` ticks stored for an environment whose episode
        still runs mature in place: reward ``+= gamma**j * reward[i]``, next_state becomes this
        tick's, not_done ``gamma**j * (1 - done[i])``.  Every ring row is at every moment an exact
        m-step transition (1 <= m <= n) for a learner whose ``discount`` is ``gamma``; ``sample``
        returns the fractional not_done as stored.  ``ended`` (bool or uint8 ``[rows]``) marks the rows
        whose episode ended with this transition, time limits included.  CUDA tensors only.  Any other
        write of the ring, or another ``rows`` / ``n`` / ``gamma``, starts a fresh lane."""
        self._add_batch_nstep((state, action, next_state, reward, done), ended, n, gamma)


class ReplayBuffer_particles(_RingBuffer):
    """Particle-observation replay ring (my_replay_buffer.py:6-69) resident in HBM.

    ``obs_space`` is the reference's 2-tuple of Boxes: features ``[F]`` and particles
    ``[N, D]`` (TD3_particles.py:29, :37); a state is the tuple ``(features, particles)``.
    One fp32 record per transition holds both states; the learner's encoders read the
    particle blocks in place, so ``TD3.train`` moves no particle bytes for sampling.
    """

    store_np = ["state_features", "state_particles", "action", "next_state_features",
                "next_state_particles", "reward", "not_done"]
    _C = {"create": "rb_create_particles", "add": "rb_add_particles", "add_device": "rb_add_particles_device",
          "add_device_hindsight": "rb_add_particles_device_hindsight",
          "add_device_nstep": "rb_add_particles_device_nstep", "sample": "rb_sample_particles"}
    _count = "seven"
    _relabel = ((0, 3), 5)
    _stage_rows = max(1, _STAGE_ROWS // 16)

    def _read_spaces(self, obs_space, action_space):
        self.feat_dim = int(obs_space[0].shape[0])
        self.n_particles, self.particle_dim = (int(x) for x in obs_space[1].shape)
        self.action_dim = int(action_space.shape[0])

    def _dims(self):
        return self.feat_dim, self.n_particles, self.particle_dim, self.action_dim

    def _row_shapes(self):
        F, N, D, A = self._dims()
        return (F,), (N, D), (A,), (F,), (N, D), (1,), (1,)

    def _dims_from(self, arrs):
        self.feat_dim = arrs["state_features"].shape[1]
        self.n_particles, self.particle_dim = arrs["state_particles"].shape[1:3]
        self.action_dim = arrs["action"].shape[1]

    def add(self, state, action, next_state, reward, done):
        """my_replay_buffer.py:46-56 (state = (features, particles); stores 1 - done)."""
        row = self._stage[self._n]
        cf, cp, ca, cf2, cp2, cr, cnd = self._cols
        nd = (self.n_particles, self.particle_dim)
        row[cf] = state[0]
        row[cp].reshape(nd)[...] = state[1]
        row[ca] = action
        row[cf2] = next_state[0]
        row[cp2].reshape(nd)[...] = next_state[1]
        row[cr] = reward
        row[cnd] = 1. - np.asarray(done, dtype=np.float64)
        if self._shadow is not None:
            self._shadow.put((state[0], state[1], action, next_state[0], next_state[1], reward, 1. - done))
        self._n += 1
        if self._n == len(self._stage):
            self.flush()

    def add_batch(self, feat, part, action, next_feat, next_part, reward, done):
        """Bulk add of n transitions.  Torch CUDA tensors (a GPU-resident environment's rows, any
        float dtype; particles ``[n][N][D]`` or ``[n][N*D]``) go from device memory straight into
        the ring (``rb_add_particles_device``): no host copy, no synchronisation."""
        self._add_batch(feat, part, action, next_feat, next_part, reward, done)

    def add_batch_hindsight(self, feat, part, action, next_feat, next_part, reward, done, *, goal_cols, goals,
                            rewards):
        """``ReplayBuffer_featured.add_batch_hindsight`` for particle transitions: the relabels write
        ``goals`` into columns ``goal_cols`` of feat and next_feat and ``rewards`` into the reward;
        the particle blocks, the action and done are the source transition's.  On CUDA tensors
        ``rb_add_particles_device_hindsight`` reads each source row once and stores it 1 + K times."""
        self._add_batch_hindsight((feat, part, action, next_feat, next_part, reward, done), goal_cols, goals,
                                  rewards)

    def add_batch_nstep(self, feat, part, action, next_feat, next_part, reward, done, *, ended, n, gamma):
        """``ReplayBuffer_featured.add_batch_nstep`` for particle transitions
        (``rb_add_particles_device_nstep``): a maturing row receives this tick's next_feat and
        next_particles; its feat, particles and action stay.  Each source row is read once per tick."""
        self._add_batch_nstep((feat, part, action, next_feat, next_part, reward, done), ended, n, gamma)


# The reference's module-level alias used by main.py:204-208.
ReplayBuffer = ReplayBuffer_featured


class MixedReplay(object):
    """Demonstration replay ("symmetric sampling": DDPGfD, RLPD): two device rings of one kind and
    dims, ``demo`` holding demonstrations (``experience_injection.py``'s rows, a ``--load_replay_buffer``
    folder) and ``online`` the rows the learner collects.  Every batch draws ``n_demo(batch)`` rows
    from ``demo`` and the rest from ``online``, so the demonstrations' share neither decays with the
    online ring's fill nor ends when a FIFO overwrites them.  ``TD3.train`` / ``train_step`` given a
    ``MixedReplay`` take the step on the device (``td3_train_step_mixed``: one input launch reads both
    rings); everything that adds rows forwards to ``online``, so ``DeviceTrainLoop`` / ``TrainLoop``
    take one unchanged.  ``demo_fraction`` is a plain attribute in [0, 1]: anneal it between steps.
    State normalisation is the rings' own: ``stats = mix.demo.state_moments()``,
    ``mix.demo.normalize_states(stats)``, and the online rows through
    ``NormalizedVecEnv(env, stats.frozen_copy(env.n_envs), norm_reward=False, update=False)``."""

    prioritized = False

    def __init__(self, online, demo, demo_fraction=0.5):
        for name, ring in (("online", online), ("demo", demo)):
            if not isinstance(ring, (ReplayBuffer_featured, ReplayBuffer_particles)):
                raise ValueError(f"MixedReplay: {name} must be a ReplayBuffer_featured or ReplayBuffer_particles")
        if type(online) is not type(demo):
            raise ValueError("MixedReplay: online and demo must be rings of the same kind")
        if online is demo:
            raise ValueError("MixedReplay: online and demo must be two rings")
        if tuple(online._dims()) != tuple(demo._dims()):
            raise ValueError(f"MixedReplay: ring dims differ (online {tuple(online._dims())}, "
                             f"demo {tuple(demo._dims())})")
        if online.device != demo.device:
            raise ValueError("MixedReplay: the rings live on different devices")
        if online.prioritized or demo.prioritized:
            raise ValueError("MixedReplay: a prioritized ring (enable_priorities): the mixed draw is uniform")
        self.online, self.demo = online, demo
        self.demo_fraction = demo_fraction
        self.device = online.device

    # ------------------------------------------------------------------ the batch split
    def n_demo(self, batch):
        return mixed_n_demo(int(batch), self.demo_fraction, self.online.size, self.demo.size)

    def _split_indices(self, batch, indices):
        """``(n_demo, idx[batch] or None)`` of a step: ``indices`` None (the device draws), an array
        ``[batch]`` split by ``n_demo(batch)``, or a pair ``(idx_demo, idx_online)`` whose lengths fix it."""
        B = int(batch)
        if indices is None:
            return self.n_demo(B), None
        if isinstance(indices, tuple) and len(indices) == 2:
            d, o = (np.asarray(x, dtype=np.int64).reshape(-1) for x in indices)
            if d.size + o.size != B:
                raise ValueError(f"indices: {d.size} demo + {o.size} online rows for a batch of {B}")
            return int(d.size), np.ascontiguousarray(np.concatenate([d, o]))
        return self.n_demo(B), np.ascontiguousarray(np.asarray(indices, dtype=np.int64).reshape(B))

    def sample(self, batch_size):
        """``demo.sample(n_demo)`` followed by ``online.sample(batch - n_demo)``, field by field: what a
        foreign learner (the reference's own ``TD3``) trains on."""
        torch = _torch()
        B = int(batch_size)
        nd = self.n_demo(B)
        parts = ([self.demo.sample(nd)] if nd else []) + ([self.online.sample(B - nd)] if B - nd else [])
        return tuple(torch.cat(f, dim=0) for f in zip(*parts))

    # ------------------------------------------------------------------ forwarded to the online ring
    def add(self, *a, **k):
        return self.online.add(*a, **k)

    def add_batch(self, *a, **k):
        return self.online.add_batch(*a, **k)

    def add_batch_hindsight(self, *a, **k):
        return self.online.add_batch_hindsight(*a, **k)

    def add_batch_nstep(self, *a, **k):
        return self.online.add_batch_nstep(*a, **k)

    def flush(self, stream=None):
        self.online.flush(stream)
        self.demo.flush(stream)

    @property
    def size(self):
        return self.online.size

    @property
    def ptr(self):
        return self.online.ptr

    def save(self, folder):
        """The online ring in the reference's layout (the demonstrations have their own folder)."""
        return self.online.save(folder)


def mixed_n_demo(batch, demo_fraction, online_size, demo_size):
    """Rows of a ``batch`` a ``MixedReplay`` draws from its demo ring: ``floor(batch * demo_fraction + 0.5)``
    capped at ``batch``; 0 while the demo ring is empty and ``batch`` while the online ring is (training
    starts at tick 0 on loaded demonstrations, ``--load_replay_buffer``'s ``start_training = 0``)."""
    f = float(demo_fraction)
    if not 0.0 <= f <= 1.0:
        raise ValueError(f"demo_fraction must be in [0, 1], got {demo_fraction!r}")
    if demo_size == 0 and online_size == 0:
        raise ValueError("MixedReplay: both rings are empty")
    if demo_size == 0:
        return 0
    if online_size == 0:
        return batch
    return min(batch, int(math.floor(batch * f + 0.5)))
