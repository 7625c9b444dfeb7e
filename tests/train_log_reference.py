"""numpy restatement of one training-log entry (include/td3.h, "training log"; train_log_kernel), in
exactly the kernel's order: fp64 on the fp32 values widened, thread p of 256 accumulating the elements (or
rows) p, p + 256, ... in increasing order from 0.0, the 256 partials combined by the halving tree
partial[p] += partial[p + s] for s = 128, 64, ..., 1; min / max by the same partition and tree with
< / >, threads without an element carrying +inf / -inf; a mean is the tree's sum divided once."""
import numpy as np

THREADS = 256
FIELDS = ("critic_loss", "actor_loss", "q1_mean", "q2_mean", "y_mean", "q_min", "q_max", "y_min", "y_max",
          "q_gap_mean", "td_abs_mean", "td_abs_max", "w_mean", "w_min")
# what follows from y, q1 and q2 alone
FROM_Q = ("q1_mean", "q2_mean", "y_mean", "q_min", "q_max", "y_min", "y_max", "q_gap_mean", "td_abs_mean",
          "td_abs_max", "nonfinite")


def _rounds(x, fill):
    """x (1-D fp64) as [rounds][256]: round k holds what the 256 threads take in their k-th turn."""
    x = np.asarray(x, np.float64).reshape(-1)
    k = max((x.size + THREADS - 1) // THREADS, 1)
    out = np.full(k * THREADS, fill, np.float64)
    out[:x.size] = x
    return out.reshape(k, THREADS)


def _tree(part, op):
    part = part.copy()
    s = THREADS // 2
    while s >= 1:
        part[:s] = op(part[:s], part[s:2 * s])
        s //= 2
    return part[0]


def _add(a, b):
    return a + b


def _lt(a, b):                 # partial[p + s] < partial[p] ? partial[p + s] : partial[p]
    return np.where(b < a, b, a)


def _gt(a, b):
    return np.where(b > a, b, a)


def fixed_sum(x):
    acc = np.zeros(THREADS, np.float64)
    for row in _rounds(x, 0.0):           # adding the 0.0 of a thread without an element changes nothing
        acc = acc + row
    return _tree(acc, _add)


def fixed_min(*xs):
    """Each thread visits its element of xs[0], then of xs[1], ..., then moves on."""
    acc = np.full(THREADS, np.inf)
    for rows in zip(*[_rounds(x, np.inf) for x in xs]):
        for row in rows:
            acc = _lt(acc, row)
    return _tree(acc, _lt)


def fixed_max(*xs):
    acc = np.full(THREADS, -np.inf)
    for rows in zip(*[_rounds(x, -np.inf) for x in xs]):
        for row in rows:
            acc = _gt(acc, row)
    return _tree(acc, _gt)


def entry(y, q1, q2=None, sqerr=None, aq=None, w=None):
    """One entry's fields as a dict.  y, q1, q2, aq: [B][nq] float32 (q2 None without a twin, aq None on a
    critic-only step); sqerr: [J][B] float32 rows of squared errors (None: critic_loss is left out);
    w: [B] float32 importance weights of a prioritized step (None: exactly 1.0)."""
    y = np.asarray(y, np.float32)
    B = y.shape[0]
    y = y.reshape(B, -1)
    nq = y.shape[1]
    n = B * nq
    q1 = np.asarray(q1, np.float32).reshape(B, nq)
    twin = q2 is not None
    q2 = np.asarray(q2, np.float32).reshape(B, nq) if twin else q1
    yd, q1d, q2d = (a.astype(np.float64) for a in (y, q1, q2))
    out = {}
    bad = (~np.isfinite(yd)).sum() + (~np.isfinite(q1d)).sum() + ((~np.isfinite(q2d)).sum() if twin else 0)
    out["nonfinite"] = int(bad)
    with np.errstate(all="ignore"):
        out["q1_mean"] = fixed_sum(q1d) / float(n)
        out["q2_mean"] = fixed_sum(q2d) / float(n)
        out["y_mean"] = fixed_sum(yd) / float(n)
        out["q_gap_mean"] = fixed_sum(np.abs(q1d - q2d)) / float(n)
        out["q_min"] = fixed_min(q1d, q2d)
        out["q_max"] = fixed_max(q1d, q2d)
        out["y_min"] = fixed_min(yd)
        out["y_max"] = fixed_max(yd)
        # t_r: each critic's sum over o in increasing order from 0.0, the critics added in order j, then
        # one product by 1 / (J * A)
        t = np.zeros(B, np.float64)
        for o in range(nq):
            t = t + np.abs(q1d[:, o] - yd[:, o])
        if twin:
            t2 = np.zeros(B, np.float64)
            for o in range(nq):
                t2 = t2 + np.abs(q2d[:, o] - yd[:, o])
            t = t + t2
        t = t * (1.0 / float((2 if twin else 1) * nq))
        out["td_abs_mean"] = fixed_sum(t) / float(B)
        out["td_abs_max"] = fixed_max(t)
        if sqerr is not None:
            sq = np.asarray(sqerr, np.float32).reshape(-1, B).astype(np.float64)
            out["critic_loss"] = fixed_sum(sq[0]) / float(n)
            if twin:
                out["critic_loss"] = out["critic_loss"] + fixed_sum(sq[1]) / float(n)
        if aq is None:
            out["actor_loss"] = float("nan")
        else:
            out["actor_loss"] = -fixed_sum(np.asarray(aq, np.float32).reshape(B, nq).astype(np.float64)) / float(n)
        if w is None:
            out["w_mean"] = out["w_min"] = 1.0
        else:
            wd = np.asarray(w, np.float32).reshape(B).astype(np.float64)
            out["w_mean"] = fixed_sum(wd) / float(B)
            out["w_min"] = fixed_min(wd)
    return {k: (v if k == "nonfinite" else float(v)) for k, v in out.items()}
