"""The learner's training log (include/td3.h, "training log").

``TrainLog`` is the host's view of the ring of per-step entries a learner keeps in device memory once
``enable_train_log`` was called: critic and actor loss, the level of Q1 / Q2 against the target y, the
twins' disagreement, the size of the TD errors, the spread of the importance weights and a count of
non-finite values, one entry per logged step, written by one small kernel behind the step and read
only when asked -- e.g. from ``DeviceTrainLoop``'s ``on_log``::

    policy.enable_train_log(capacity=4096, every=16)
    loop = DeviceTrainLoop(env, policy, rb, log_every=1000,
                           on_log=lambda t, info: print(t, policy.train_log.summary(last=64)))
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

__all__ = ["TrainLog", "ENTRY_DTYPE"]

# td3_log_entry of include/td3.h
ENTRY_DTYPE = np.dtype([("step", "<i8"), ("batch", "<i4"), ("actor_step", "<i4"), ("prioritized", "<i4"),
                        ("nonfinite", "<i4"), ("critic_loss", "<f8"), ("actor_loss", "<f8"), ("q1_mean", "<f8"),
                        ("q2_mean", "<f8"), ("y_mean", "<f8"), ("q_min", "<f8"), ("q_max", "<f8"), ("y_min", "<f8"),
                        ("y_max", "<f8"), ("q_gap_mean", "<f8"), ("td_abs_mean", "<f8"), ("td_abs_max", "<f8"),
                        ("w_mean", "<f8"), ("w_min", "<f8")])
_MEANS = ("critic_loss", "q1_mean", "q2_mean", "y_mean", "q_gap_mean", "td_abs_mean", "w_mean")


class TrainLog:
    """The training log of one learner (``policy.train_log`` after ``policy.enable_train_log``)."""

    def __init__(self, policy, capacity=4096, every=1):
        self._lib = policy._lib
        if C.sizeof(_lib.td3_log_entry) != self._lib.td3_log_entry_size() or \
                ENTRY_DTYPE.itemsize != C.sizeof(_lib.td3_log_entry):
            raise _lib.TD3Error(f"td3_log_entry binding is {C.sizeof(_lib.td3_log_entry)} bytes, libtd3hip's "
                                f"{self._lib.td3_log_entry_size()}: td3_amd/_lib.py is out of date with include/td3.h")
        check(self._lib.td3_log_enable(policy._h, int(capacity), int(every)), "td3_log_enable")
        self._policy = policy                 # the handle's owner: the log lives as long as the learner
        self.capacity, self.every = int(capacity), int(every)

    # ------------------------------------------------------------------ reading
    def info(self):
        inf = _lib.td3_log_info_t()
        check(self._lib.td3_log_info(self._policy._h, C.byref(inf)), "td3_log_info")
        return inf

    @property
    def count(self):
        """Steps logged so far (the next sequence number); no synchronisation."""
        return int(self.info().count)

    def read(self, first=None, n=None):
        """``(first_seq, entries)``: the entries with sequence numbers in ``[first, first + n)`` that are
        still in the ring (the last ``capacity``), oldest first, and the sequence number of the first
        one.  Waits for the last logged step only."""
        first = 0 if first is None else int(first)
        n = (1 << 62) if n is None else int(n)
        raw = np.zeros(max(min(n, self.capacity), 1), ENTRY_DTYPE)
        f0, cnt = C.c_int64(), C.c_int64()
        # (the window [first, first + n) is in sequence numbers: at most `capacity` of them are in the ring)
        check(self._lib.td3_log_read(self._policy._h, first, n, raw.ctypes.data_as(C.POINTER(_lib.td3_log_entry)),
                                     C.byref(f0), C.byref(cnt)), "td3_log_read")
        return f0.value, raw[:cnt.value].copy()

    def entries(self, first=None, n=None):
        """A structured array (``ENTRY_DTYPE``: the fields of ``td3_log_entry``) of the logged steps
        ``[first, first + n)`` still in the ring, oldest first; by default everything in the ring."""
        return self.read(first, n)[1]

    def summary(self, last=None):
        """A dict over the last ``last`` entries still in the ring (all of them by default), computed
        on the host in fp64: ``steps``, ``first_step``, ``last_step``; the means of ``critic_loss``,
        ``q1_mean``, ``q2_mean``, ``y_mean``, ``q_gap_mean``, ``td_abs_mean``, ``w_mean``; the mean of
        ``actor_loss`` over the actor steps (NaN without one); the max of ``td_abs_max``; the min of
        ``w_min``; the sum of ``nonfinite``."""
        e = self.entries()
        if last is not None:
            e = e[max(len(e) - int(last), 0):]
        return summarize(e)

    # ------------------------------------------------------------------ state
    def state_dict(self):
        """The entries still in the ring and the counters, as numpy values."""
        first, e = self.read()
        return {"entries": e, "count": np.int64(first + len(e)), "capacity": np.int64(self.capacity),
                "every": np.int64(self.every)}

    def load_state_dict(self, sd):
        """Restore a ``state_dict``: the last ``capacity`` of its entries and its count.  A run
        continued from here reads back what the uninterrupted run does."""
        e = np.ascontiguousarray(np.asarray(sd["entries"], ENTRY_DTYPE).reshape(-1)[-self.capacity:])
        check(self._lib.td3_log_set(self._policy._h, e.ctypes.data_as(C.POINTER(_lib.td3_log_entry)), len(e),
                                    int(sd["count"])), "td3_log_set")

    def save(self, path):
        """The ``state_dict`` as one ``.npz``."""
        np.savez(path, **self.state_dict())

    def load(self, path):
        with np.load(path) as z:
            self.load_state_dict({k: z[k] for k in z.files})


def summarize(e):
    """``TrainLog.summary`` of a structured array of entries."""
    out = {"steps": int(len(e)), "first_step": int(e["step"][0]) if len(e) else None,
           "last_step": int(e["step"][-1]) if len(e) else None}
    nan = float("nan")
    for k in _MEANS:
        out[k] = float(np.mean(e[k], dtype=np.float64)) if len(e) else nan
    act = e["actor_loss"][e["actor_step"] != 0]
    out["actor_loss"] = float(np.mean(act, dtype=np.float64)) if len(act) else nan
    out["td_abs_max"] = float(np.max(e["td_abs_max"])) if len(e) else nan
    out["w_min"] = float(np.min(e["w_min"])) if len(e) else nan
    out["nonfinite"] = int(np.sum(e["nonfinite"], dtype=np.int64))
    return out
