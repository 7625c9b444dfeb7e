"""A numpy fp64 restatement of one rollout-statistics tick (include/td3.h, "rollout statistics"):
the four steps in the header's order.  The batch sums use numpy's own summation order; the tests
bound the difference to the device's fixed order by the fp64 summation bound."""
import numpy as np


def chan_merge(count, mean, m2, x):
    """Merge the rows of ``x`` ([n] or [n][d]) into running moments; returns the new triple."""
    n = x.shape[0]
    mb = x.sum(axis=0) / n
    m2b = ((x - mb) ** 2).sum(axis=0)
    delta, tot = mb - mean, count + n
    return tot, mean + delta * n / tot, m2 + m2b + delta * delta * count * n / tot


def normalise(x, count, mean, m2, eps, clip, mask=None):
    """Step 2 for fp32 rows ``x``: fp64 arithmetic, one rounding to fp32; masked columns and
    ``count == 0`` pass ``x`` through."""
    x = np.asarray(x, np.float32)
    if count == 0:
        return x.copy()
    y = np.clip((x.astype(np.float64) - mean) / np.sqrt(m2 / count + eps), -clip, clip).astype(np.float32)
    return y if mask is None else np.where(np.asarray(mask) != 0, y, x)


def scale_reward(r, ret_count, ret_m2, eps, clip):
    r = np.asarray(r, np.float32)
    if ret_count == 0:
        return r.copy()
    return np.clip(r.astype(np.float64) / np.sqrt(ret_m2 / ret_count + eps), -clip, clip).astype(np.float32)


class RolloutStatsRef:
    def __init__(self, rows, obs_dim, *, gamma, obs_clip=10.0, rew_clip=10.0, eps=1e-8, col_mask=None, log_cap=4096):
        self.rows, self.obs_dim, self.log_cap = rows, obs_dim, log_cap
        self.gamma, self.obs_clip, self.rew_clip, self.eps = gamma, obs_clip, rew_clip, eps
        self.mask = np.ones(obs_dim, bool) if col_mask is None else np.asarray(col_mask) != 0
        self.count, self.mean, self.m2 = 0.0, np.zeros(obs_dim), np.zeros(obs_dim)
        self.ret_count, self.ret_mean, self.ret_m2 = 0.0, 0.0, 0.0
        self.G, self.ep_return, self.ep_len = np.zeros(rows), np.zeros(rows), np.zeros(rows, np.int32)
        self.log = [None] * log_cap           # slot -> (ret fp32, len, row, tick)
        self.ep_count, self.ep_return_sum, self.ep_len_sum, self.tick_no = 0, 0.0, 0, 0

    def tick(self, obs=None, next_obs=None, reward=None, ended=None, update=True):
        out = [None, None, None]
        if update and obs is not None:                                              # 1
            x = np.asarray(obs, np.float32).astype(np.float64)
            self.count, mean, m2 = chan_merge(self.count, self.mean, self.m2, x)
            self.mean, self.m2 = np.where(self.mask, mean, 0.0), np.where(self.mask, m2, 0.0)
        for j, x in enumerate((obs, next_obs)):                                     # 2
            if x is not None:
                out[j] = normalise(x, self.count, self.mean, self.m2, self.eps, self.obs_clip, self.mask)
        if reward is not None:
            r = np.asarray(reward, np.float32)
            e = np.zeros(self.rows, bool) if ended is None else np.asarray(ended) != 0
            self.G = self.gamma * self.G + r.astype(np.float64)                     # 3
            if update:
                self.ret_count, self.ret_mean, self.ret_m2 = chan_merge(self.ret_count, self.ret_mean, self.ret_m2,
                                                                        self.G)
            out[2] = scale_reward(r, self.ret_count, self.ret_m2, self.eps, self.rew_clip)
            self.G[e] = 0.0
            self.ep_return += r.astype(np.float64)                                  # 4
            self.ep_len += 1
            for i in np.flatnonzero(e):
                self.log[self.ep_count % self.log_cap] = (np.float32(self.ep_return[i]), int(self.ep_len[i]), int(i),
                                                          self.tick_no)
                self.ep_count += 1
                self.ep_return_sum += self.ep_return[i]
                self.ep_len_sum += int(self.ep_len[i])
                self.ep_return[i], self.ep_len[i] = 0.0, 0
            self.tick_no += 1
        return tuple(out)

    def episodes(self):
        """The entries still in the ring, oldest first."""
        lo = max(0, self.ep_count - self.log_cap)
        return [self.log[k % self.log_cap] for k in range(lo, self.ep_count)]
