"""Exploration noise for the acting loop.

The reference perturbs ``select_action`` with an Ornstein-Uhlenbeck process
(``utils/noise.py:4-22``, used at ``main.py:240,251-253``): per environment step

    X <- X + (theta * (mu - X) + sigma * n),   n ~ N(0, I) from numpy's global RNG,

and ``reset()`` at episode ends returns X to mu.  It is a few flops per step, so it stays on the
host beside ``env.step``.  The update below keeps the reference's rounding order (drift first,
then the diffusion term, then the add), so a seeded numpy RNG gives the same float64 sequence.
"""
from __future__ import annotations

import numpy as np

__all__ = ["OrnsteinUhlenbeckActionNoise", "DeviceOUNoise", "DeviceGaussianNoise"]


class OrnsteinUhlenbeckActionNoise:
    """Drop-in for the reference class: ``(action_dim, mu=0, theta=0.1, sigma=0.2)``,
    ``sample() -> float64 [action_dim]``, ``reset()``; the state is exposed as ``X``."""

    def __init__(self, action_dim, mu=0, theta=0.1, sigma=0.2):
        self.action_dim = int(action_dim)
        self.mu, self.theta, self.sigma = mu, theta, sigma
        self.reset()

    def reset(self):
        self.X = np.full(self.action_dim, self.mu, dtype=np.float64)

    def sample(self):
        drift = self.theta * (self.mu - self.X)
        step = drift + self.sigma * np.random.randn(self.action_dim)
        self.X = self.X + step
        return self.X


class DeviceOUNoise:
    """The same process for ``n_envs`` environments at once, resident on the GPU: ``X`` is a float32
    ``[n_envs][action_dim]`` device tensor that ``TD3.select_action_device(states, noise=self)``
    updates in the policy query's own epilogue kernel (``explore_kernel``), drawing N(0, 1) from a
    Philox stream keyed by ``seed`` and counted by ``step`` (one per query; include/td3.h gives the
    counter layout).  fp32 on the device where the host class is float64: a deliberate difference.

    ``reset(mask=None)`` returns every row (or the rows where the ``[n_envs]`` mask is nonzero) to
    ``mu`` with a torch op; passing the mask as ``select_action_device(..., reset=mask)`` instead
    applies it inside the kernel."""

    def __init__(self, n_envs, action_dim, mu=0, theta=0.1, sigma=0.2, device=None, seed=0):
        import torch
        self.n_envs, self.action_dim = int(n_envs), int(action_dim)
        self.mu, self.theta, self.sigma = float(mu), float(theta), float(sigma)
        self.device = torch.device("cuda") if device is None else torch.device(device)
        self.seed, self.step = int(seed), 0
        self.X = torch.full((self.n_envs, self.action_dim), self.mu, dtype=torch.float32, device=self.device)

    def reset(self, mask=None):
        if mask is None:
            self.X.fill_(self.mu)
        else:
            self.X.masked_fill_(mask.to(self.device).reshape(-1, 1) != 0, self.mu)


class DeviceGaussianNoise:
    """Uncorrelated exploration on the device: ``a = clip(pi + sigma * z)``, ``z`` from the same
    Philox stream (``td3_explore`` with no OU state)."""

    X = None
    mu, theta = 0.0, 0.0

    def __init__(self, sigma=0.1, seed=0):
        self.sigma = float(sigma)
        self.seed, self.step = int(seed), 0

    def reset(self, mask=None):
        pass
