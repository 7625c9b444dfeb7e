"""The float64 reference of the featured query path and the table of planner-edge cases.

TEST INFRASTRUCTURE ONLY (no GPU, nothing in ``td3_amd/`` imports it).  Used by
``tests/test_query_reference.py`` (CPU: the table covers what it claims, the tolerance is attainable,
the comparison can fail) and ``tests/test_gpu_query_edges.py`` (the HIP query kernels against it).

``forward64`` is the independent side of the comparison: it restates the featured MLP
(TD3_featured.py:41-46 / :75-80: Linear -> ReLU -> LayerNorm on the three hidden layers, a bare last
Linear) in float64 and never calls ``oracle/td3_oracle.py``.

Every case fixes the shapes at which ``build_act`` / ``run_gemv`` / ``launch_act`` (td3_amd/csrc/act.hip,
kernels_launch.h) take another branch.  ``route`` holds, written out by hand, the string
``td3_debug_query_route`` must give for a query of n <= 4 rows (``{R}`` is the rows a wave holds:
``ROWS_OF_N``); it is NOT computed from the shapes, so that a planner that silently picks another kernel
fails the GPU suite instead of being followed by it.
"""
from __future__ import annotations

import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(_HERE, "golden"),):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gen  # noqa: E402

f64 = np.float64
LN_EPS = 1e-5
POOL_ROWS = 257
TOL = 1e-5                       # SURVEY §8c forward contract, relative to scale(case, head)
HEADS = ("action", "q1", "q2")

DEFAULT = (gen.ACTOR_ARCH, gen.Q_ARCH)        # (500, 400, 300) / (500, 400, 200)
ODD = ((64, 48, 40), (96, 72, 33))

# template argument R of the small-query kernels for n live rows (3 rows run R = 4 with one dead row)
ROWS_OF_N = {1: 1, 2: 2, 3: 4, 4: 4}

_ACT8 = "args,td3::act_kernel<{R}, 8>"
_ACT16 = "args,td3::act_kernel<{R}, 16>"
_CHAIN01 = "args,td3::gemv01_kernel<{R}>,td3::gemv_kernel<{R}>,td3::head_kernel"
_CHAIN = "mapped,td3::gemv_kernel<{R}>,td3::gemv_kernel<{R}>,td3::gemv_kernel<{R}>,td3::head_kernel"


def _case(sd, ad, widths, norm, seed, act, q, ma=1.0):
    return dict(sd=sd, ad=ad, actor_arch=tuple(widths[0]), q_arch=tuple(widths[1]), norm=norm, seed=seed,
                ma=ma, route={"act": act, "q": q})


# name: shapes, norm, the pool seed (chosen so that every applicable mutation shows on the first four
# pool rows, tests/test_query_reference.py asserts it) and the n <= 4 route of select_action / eval_q
CASES = {
    # K0 = 1 and 2: the query rows overlap inside a float4; nout = 1
    "min": _case(1, 1, DEFAULT, "layer", 1, _ACT8, _ACT8, ma=2.0),
    # critic K0 = 32: the last KQ = 8
    "k32": _case(26, 6, DEFAULT, "layer", 2, _ACT8, _ACT8),
    # critic K0 = 33: the first KQ = 16 (the actor stays 8)
    "k33": _case(27, 6, DEFAULT, "layer", 3, _ACT8, _ACT16),
    # KQ 16 / 16; the head's tail loop (nout = 17 > 8 preloaded rows of W4)
    "a17": _case(40, 17, DEFAULT, "layer", 4, _ACT16, _ACT16, ma=0.4),
    # actor K0 = 32, critic K0 = 64 (a full layer-0 row); nout = 32
    "k64_a32": _case(32, 32, DEFAULT, "layer", 5, _ACT8, _ACT16, ma=0.5),
    # critic K0 = 65: no gemv01, gemv_kernel x 3 + head for BOTH networks, rows in mapped memory
    "k65": _case(33, 32, DEFAULT, "layer", 6, _CHAIN, _CHAIN),
    # actor K0 = 64 would fit, the critic's 65 does not: the chain for both
    "s64": _case(64, 1, DEFAULT, "layer", 7, _CHAIN, _CHAIN),
    # the chain at K = 512 (both float4 halves of a lane's slice full)
    "in512": _case(480, 32, DEFAULT, "layer", 8, _CHAIN, _CHAIN, ma=0.4),
    # nb = 3 and 5, ragged last groups (48, 72), layer 2 with idle workgroups (40), a one-column wave (33)
    "odd": _case(11, 3, ODD, "layer", 9, _ACT8, _ACT8),
    "odd_none": _case(11, 3, ODD, None, 10, _ACT8, _ACT8),
    # the derived W (g v / |v|) read by the query kernels
    "odd_wn": _case(11, 3, ODD, "weight_normalization", 11, _ACT8, _ACT8),
    # nb = 1 (poll and last arriver are one workgroup); LN over 5 columns; critic N2 == N1
    "one_wg": _case(17, 6, ((20, 12, 5), (24, 16, 16)), "layer", 12, _ACT8, _ACT8),
    # rides() false (N2 > N1): gemv01 + gemv + head in production
    "grow": _case(17, 6, ((64, 48, 80), (64, 48, 80)), "layer", 13, _CHAIN01, _CHAIN01),
    # only the critic fails rides(): the actor leaves the one-launch route too (act1 is one flag per plan)
    "grow_q": _case(17, 6, ((64, 48, 40), (64, 48, 80)), "layer", 14, _CHAIN01, _CHAIN01),
    # N0 = 512, nb = 32, no pad anywhere
    "wide": _case(17, 6, ((512, 512, 512), (512, 512, 512)), "layer", 15, _ACT8, _ACT8),
    # widths % 4 != 0 near the top of the second float4 half; a last group of 13 columns
    "w510": _case(17, 6, ((510, 509, 507), (510, 509, 507)), "layer", 16, _ACT8, _ACT8),
}


def expected_route(case, n, which):
    """The literal ``td3_debug_query_route`` string of a host query of n <= 4 rows (which: "act" / "q")."""
    return CASES[case]["route"][which].format(R=ROWS_OF_N[n])


def pad32(k):
    return (k + 31) // 32 * 32


def params(case):
    """(actor, critic) state dicts of a case, as tests/test_gpu_edges.py::_setup draws them."""
    c = CASES[case]
    sd, ad, norm = c["sd"], c["ad"], c["norm"]
    a0 = gen.init_params(gen._mlp_shapes("", sd, c["actor_arch"], ad, norm), gen.SEED)
    c0 = gen.init_params(gen._mlp_shapes("q1.", sd + ad, c["q_arch"], 1, norm) +
                         gen._mlp_shapes("q2.", sd + ad, c["q_arch"], 1, norm), gen.SEED + 100)
    return a0, c0


def pool(case):
    """(states [257][sd], actions [257][ad]) float32 of a case; a query of n rows uses the first n."""
    c = CASES[case]
    rs = np.random.RandomState(1000 + c["seed"])
    s = rs.standard_normal((POOL_ROWS, c["sd"])).astype(np.float32)
    a = rs.uniform(-c["ma"], c["ma"], size=(POOL_ROWS, c["ad"])).astype(np.float32)
    return s, a


# ------------------------------------------------------------------ mutations
# Wrong-on-purpose variants of forward64, each the error a kernel would make at one of the edges:
#   ("ln_pad", i)    LayerNorm of hidden layer i divides by pad32(K) instead of K
#   ("drop_col", i)  the last real column of hidden layer i is dropped (reads as zero)
#   ("head_row7",)   head outputs o >= 8 computed with row 7 of W4 (the preloaded rows only)
#   ("row0",)        query row r > 0 reads row 0's input
#   ("drop_in",)     layer-0 input column K0 - 1 dropped
MUTATIONS = {
    "a0": ("ln_pad", 0), "a1": ("ln_pad", 1), "a2": ("ln_pad", 2),
    "b0": ("drop_col", 0), "b1": ("drop_col", 1), "b2": ("drop_col", 2),
    "c": ("head_row7",), "d": ("row0",), "e": ("drop_in",),
}


def applies(case, mut, net):
    """Whether mutation ``mut`` changes anything in network ``net`` ("actor" / "q") of a case with
    n >= 2 rows: (a) needs a LayerNorm over a width that is no multiple of 32, (c) more than 8 outputs."""
    c = CASES[case]
    kind = MUTATIONS[mut]
    arch = c["actor_arch"] if net == "actor" else c["q_arch"]
    if kind[0] == "ln_pad":
        return c["norm"] == "layer" and arch[kind[1]] % 32 != 0
    if kind[0] == "head_row7":
        return net == "actor" and c["ad"] > 8
    return True


def _linear(P, prefix, norm, i):
    b = np.asarray(P[f"{prefix}linears.{i}.bias"], f64)
    if norm == "weight_normalization":
        g = np.asarray(P[f"{prefix}linears.{i}.weight_g"], f64)
        v = np.asarray(P[f"{prefix}linears.{i}.weight_v"], f64)
        return g * v / np.sqrt((v * v).sum(axis=1, keepdims=True)), b
    return np.asarray(P[f"{prefix}linears.{i}.weight"], f64), b


def forward64(P, prefix, norm, x, mut=None):
    """The featured MLP ``prefix`` of state dict ``P`` on rows ``x`` in float64: the last Linear's
    output [n][nout].  ``mut`` (a MUTATIONS key) makes it wrong on purpose."""
    kind = MUTATIONS[mut] if mut else (None,)
    a = np.array(x, dtype=f64)
    if kind[0] == "row0":
        a = np.repeat(a[:1], a.shape[0], axis=0)
    if kind[0] == "drop_in":
        a[:, -1] = 0.0
    for i in range(4):
        W, b = _linear(P, prefix, norm, i)
        if i == 3:
            if kind[0] == "head_row7" and W.shape[0] > 8:
                W = W.copy()
                W[8:] = W[7]
            return a @ W.T + b
        h = np.maximum(a @ W.T + b, 0.0)
        if kind == ("drop_col", i):
            h[:, -1] = 0.0
        if norm == "layer":
            K = h.shape[1]
            div = pad32(K) if kind == ("ln_pad", i) else K
            mean = h.sum(axis=1, keepdims=True) / div
            var = ((h - mean) ** 2).sum(axis=1, keepdims=True) / div
            g = np.asarray(P[f"{prefix}lnorms.{i}.weight"], f64)
            be = np.asarray(P[f"{prefix}lnorms.{i}.bias"], f64)
            a = (h - mean) / np.sqrt(var + LN_EPS) * g + be
        else:
            a = h
    raise AssertionError("unreachable")


def actor64(P, norm, max_action, s, mut=None):
    return float(max_action) * np.tanh(forward64(P, "", norm, s, mut))


def q64(P, q, norm, s, a, mut=None):
    x = np.concatenate([np.asarray(s, f64), np.asarray(a, f64)], axis=1)
    return forward64(P, f"{q}.", norm, x, mut)[:, 0]


_ref_cache = {}


def reference(case):
    """{"action": [257][ad], "q1": [257], "q2": [257]} of the case's pool (Q on the pool's actions),
    computed once and shared: do not write into it."""
    if case not in _ref_cache:
        c = CASES[case]
        a0, c0 = params(case)
        s, a = pool(case)
        out = {"action": actor64(a0, c["norm"], c["ma"], s), "q1": q64(c0, "q1", c["norm"], s, a),
               "q2": q64(c0, "q2", c["norm"], s, a)}
        for v in out.values():
            v.setflags(write=False)
        _ref_cache[case] = out
    return _ref_cache[case]


def scale(case, head):
    """max |reference| of a head over the whole pool: what every tolerance is relative to."""
    return float(np.abs(reference(case)[head]).max())
