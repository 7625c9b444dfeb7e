"""The particle encoder at its edge shapes against the float64 oracle.

tests/test_gpu_particles.py runs the encoder kernels (enc_fwd_kernel<DK>, enc_gpool_kernel,
enc_bwd_kernel<DK, 2>, enc_adam_kernel) at F=7, D=9, A=3 with N=16 / B=32, 64 and N=350 / B=16
only.  The cases here start from F=7, N=16, D=9, A=3, B=32, norm="layer", CDQ and change what is
listed, on rings of 300 rows:

  case        changes                     DK ntile last  critic nwg (rows)  actor nwg (rows)  seeds
  d1          D=1                          4   1    16     32 (1..1)          32 (1..1)         1 0
  d4          D=4                          4   1    16     32 (1..1)          32 (1..1)         0 1
  d5          D=5                          8   1    16     32 (1..1)          32 (1..1)         0 2
  d8          D=8                          8   1    16     32 (1..1)          32 (1..1)         1 0
  d12         D=12                        12   1    16     32 (1..1)          32 (1..1)         0 0
  d13         D=13                        16   1    16     32 (1..1)          32 (1..1)         0 0
  d16         D=16                        16   1    16     32 (1..1)          32 (1..1)         0 0
  n1          N=1                         12   1     1     32 (1..1)          32 (1..1)         1 0
  n31         N=31                        12   1    31     32 (1..1)          32 (1..1)         0 0
  n32         N=32                        12   1    32     32 (1..1)          32 (1..1)         1 0
  n33         N=33                        12   2     1     32 (1..1)          32 (1..1)         0 0
  n65         N=65, B=8                   12   3     1      8 (1..1)           8 (1..1)         0 0
  b1          B=1                         12   1    16      1 (1..1)           1 (1..1)         0 0
  b33         B=33                        12   1    16     33 (1..1)          33 (1..1)         1 1
  b130        B=130                       12   1    16    128 (1..2)         130 (1..1)         1 0
  b257        B=257, N=33, D=5             8   2     1    128 (2..3)         256 (1..2)         0 0
  a1          A=1                         12   1    16     32 (1..1)          32 (1..1)         1 0
  f1          F=1                         12   1    16     32 (1..1)          32 (1..1)         0 0
  f352_a32    F=352, A=32 (512 columns)   12   1    16     32 (1..1)          32 (1..1)         0 1
  none_nocdq  norm=None, CDQ=False,       16   2     1     33 (1..1)          33 (1..1)         0 0
              N=33, D=13, B=33

DK is the enc_fwd_kernel / enc_bwd_kernel instantiation ((D + 3) / 4 * 4), ntile = ceil(N / 32),
"last" the valid rows of the last particle tile (32: no masked row), nwg the workgroups of
enc_bwd_kernel per network (min(B, 256 / networks in the launch): two critics, one actor) with the
shortest and longest row range [g B / nwg, (g + 1) B / nwg) among them, and "seeds" the data seeds
of part 2's critic and actor phases.  ``test_case_table_reaches_every_path`` recomputes the columns
and asserts that all four DK, single- and multi-tile N with a full, a 1-row and a 31-row last
tile, and uneven row ranges in both phases (at ntile = 2: the double-buffered tile fetch crosses
batch-row boundaries inside a workgroup) are each reached by some case.

Part 1 (``test_edge_step_teacher_forced``): two teacher-forced steps on random data, a critic-only
step then a policy step, as ``test_many_particle_tiles``, at the tolerances of ``_check_step``; the
ring gather bit-equal to the oracle buffer's (record width 2F + 2ND + A + 2, odd and unaligned
here); select_action, td3_select_action_particles on 3 observations and eval_q at rtol 1e-5 /
atol 1e-6.  This is the part that runs the actor phase on ring records.

Part 2 (``test_edge_encoder_gradients``): the gradients through both Adam moments from zero moments,
as tests/test_gpu_gradients.py reads them, at M_RTOL / V_RTOL of the float64 oracle (or no further
from it than 3x the fp32 oracle).  A comparison at 1e-4 of the tensor scale needs both sides to take
the same relu' decisions, and the particle path exports no masks.  So the encoders are put on a
dyadic grid (helpers.particle_grid_params / grid_particles) on which every conv1 / conv2
pre-activation is an odd multiple of 1/256 / 1/8192, exact in fp32 in any summation order and never
zero: the test asserts that in the float64 oracle, as a precondition of the construction.  The MLP
hidden layers keep data-dependent decisions; there the data seed of each phase is the first from 0
upward for which no hidden pre-activation of any network the phase backpropagates through (Q1, Q2
for the critic step; the actor and Q1(s, pi) for _actor_learn) lies within MASK_EPS of its layer's
max |z| of zero in the float64 oracle (the near-zero set of test_gpu_gradients._own_masks).  The
test recomputes that set and asserts that it is empty: a condition on the inputs, decided by the
oracle alone, never an exclusion of elements.  The critic gradient is that of one critic-only
train_step; the actor gradient that of ``_actor_learn`` on B grid rows from the same grid state
(inside a train step the actor phase reads the critic the step has just moved off the grid by
+- lr, which is why part 1 covers that path).

Part 3: the two refusals of td3_create for particle learners (D = 17, input width 513).
"""
import numpy as np
import pytest

from helpers import (GRID_Z1_UNIT, GRID_Z2_UNIT, gen, grid_particles, orc, particle_grid_params,
                     particle_setup_dims)
from test_gpu_gradients import (MASK_EPS, _check, _copy_learner, _Float64Oracle, _step64)
from test_gpu_parity import _load_oracle_state
from test_gpu_particles import Box, _check_step, _make

pytestmark = pytest.mark.gpu

ROWS = 300
BASE = dict(F=7, N=16, D=9, A=3, B=32, norm="layer", cdq=True)
# name: (what differs from BASE, (critic data seed, actor data seed) of part 2)
CASES = {
    "d1": (dict(D=1), (1, 0)),
    "d4": (dict(D=4), (0, 1)),
    "d5": (dict(D=5), (0, 2)),
    "d8": (dict(D=8), (1, 0)),
    "d12": (dict(D=12), (0, 0)),
    "d13": (dict(D=13), (0, 0)),
    "d16": (dict(D=16), (0, 0)),
    "n1": (dict(N=1), (1, 0)),
    "n31": (dict(N=31), (0, 0)),
    "n32": (dict(N=32), (1, 0)),
    "n33": (dict(N=33), (0, 0)),
    "n65": (dict(N=65, B=8), (0, 0)),
    "b1": (dict(B=1), (0, 0)),
    "b33": (dict(B=33), (1, 1)),
    "b130": (dict(B=130), (1, 0)),
    "b257": (dict(B=257, N=33, D=5), (0, 0)),
    "a1": (dict(A=1), (1, 0)),
    "f1": (dict(F=1), (0, 0)),
    "f352_a32": (dict(F=352, A=32), (0, 1)),
    "none_nocdq": (dict(norm=None, cdq=False, N=33, D=13, B=33), (0, 0)),
}


def _case(name):
    return dict(BASE, **CASES[name][0])


def _setup(c, seed, grid):
    """The setup of case ``c`` on ring rows drawn from ``seed``; ``grid``: particles and every
    encoder's parameters on the dyadic grid."""
    data = gen.fill_particle_buffer(c["F"], c["N"], c["D"], c["A"], ROWS, seed)
    if grid:
        f, p, a, f2, p2, r, d = data
        data = (f, grid_particles(p), a, f2, grid_particles(p2), r, d)
    S = particle_setup_dims(c["F"], c["N"], c["D"], c["A"], c["norm"], c["cdq"], c["B"], rows=ROWS, data=data)
    if grid:
        S["actor"] = particle_grid_params(S["actor"], 21)
        S["critic"] = particle_grid_params(S["critic"], 22)
    return S


# ------------------------------------------------------------------ the case table
def _paths(c):
    """What the kernels do at case ``c``: DK, ntile, valid rows of the last tile and, per phase,
    (nwg, shortest, longest row range) of enc_bwd_kernel (enc_bwd_nwg and b_begin / b_end)."""
    def ranges(nnets):
        nwg = max(1, min(c["B"], 256 // nnets))
        n = [(g + 1) * c["B"] // nwg - g * c["B"] // nwg for g in range(nwg)]
        return nwg, min(n), max(n)
    ntile = (c["N"] + 31) // 32
    return dict(DK=(c["D"] + 3) // 4 * 4, ntile=ntile, last=c["N"] - 32 * (ntile - 1),
                critic=ranges(2 if c["cdq"] else 1), actor=ranges(1))


def test_case_table_reaches_every_path():
    paths = {name: _paths(_case(name)) for name in CASES}
    assert {p["DK"] for p in paths.values()} == {4, 8, 12, 16}
    ds = {_case(name)["D"] for name in CASES}
    assert {1, 4, 8, 12, 16} <= ds                        # D = 1 and every D that fills its DK
    for last in (32, 1, 31):                               # no masked row, one valid row, one masked row
        assert any(p["last"] == last for p in paths.values()), last
    assert any(p["ntile"] == 1 and p["last"] == 1 for p in paths.values())      # N = 1
    assert any(p["ntile"] > 1 and p["last"] == 1 for p in paths.values())       # N = 33
    for phase in ("critic", "actor"):
        uneven = [p for p in paths.values() if p[phase][1] != p[phase][2]]
        assert uneven, phase
        assert any(p["ntile"] > 1 for p in uneven), (phase, "uneven ranges across tile boundaries")
    assert any(_case(name)["B"] % 32 == 1 for name in CASES)                    # 31 padding rows


# ------------------------------------------------------------------ part 1
@pytest.mark.parametrize("name", list(CASES))
def test_edge_step_teacher_forced(name):
    c = _case(name)
    F, N, D, A, B = c["F"], c["N"], c["D"], c["A"], c["B"]
    S = _setup(c, 13, grid=False)
    pol, rb = _make(S, rows=ROWS, data=S["data"])
    buf = S["buf"]
    rs = np.random.RandomState(14)

    idx = rs.randint(0, ROWS, B)
    for o, r in zip(rb.sample(B, indices=idx), buf.gather(idx)):
        np.testing.assert_array_equal(o.cpu().numpy().reshape(r.shape), r)

    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    for step in range(1, 3):
        idx = rs.randint(0, ROWS, B)
        noise = rs.standard_normal((B, A)).astype(np.float32)
        _load_oracle_state(pol, L)
        rec = orc.particle_train_step(L, buf.gather(idx), noise)
        out = pol.train_step(rb, B, indices=idx, noise=noise, stats=True)
        np.testing.assert_array_equal(out["idx"], idx)
        _check_step(out, rec, pol, L, (name, step))

    # queries on the learner the GPU now holds
    from td3_amd import _lib
    actor, critic = pol.actor.numpy_dict(), pol.critic.numpy_dict()
    f = rs.standard_normal((3, F)).astype(np.float32)
    p = rs.standard_normal((3, N, D)).astype(np.float32)
    ref, _ = orc.particle_net(actor, "", c["norm"], f, p, actor=True)
    a = pol.select_action((f[0], p[0]))
    np.testing.assert_allclose(a, ref[0], rtol=1e-5, atol=1e-6)
    out = np.empty((3, A), np.float32)
    _lib.check(pol._lib.td3_select_action_particles(pol._h, _lib.fptr(f), _lib.fptr(p), _lib.fptr(out), 3),
               "td3_select_action_particles")
    np.testing.assert_allclose(out, ref, rtol=1e-5, atol=1e-6)
    q = pol.eval_q((f[0], p[0]), a)
    qs = ("q1", "q2") if c["cdq"] else ("q1",)
    assert len(q) == len(qs)
    for j, qn in enumerate(qs):
        qr, _ = orc.particle_net(critic, f"{qn}.", c["norm"], f[:1], p[:1], a[None])
        np.testing.assert_allclose(q[j], qr[0], rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------ part 2
def _net64(P, prefix, norm, f, p, a=None, actor=False):
    """One network in the float64 oracle: its output, the pre-activations of its three hidden
    layers and those of its encoder (z1 [B N][256], z2 [B N][128])."""
    as64 = lambda x: None if x is None else np.asarray(x, np.float64)   # noqa: E731
    with _Float64Oracle():
        P64 = {k: as64(v) for k, v in P.items() if k.startswith(prefix)}
        out, cache = orc.particle_net(P64, prefix, norm, as64(f), as64(p), as64(a), actor=actor)
    (x, h1, _, _, W1, W2, _, _), _, _, _, lin, _, mlp, _, _ = cache
    zs = [mlp["u"][i] @ lin[i][0].T + lin[i][1][None, :] for i in range(3)]
    z1 = x @ W1.T + P64[f"{prefix}conv1.bias"][None, :]
    z2 = h1 @ W2.T + P64[f"{prefix}conv2.bias"][None, :]
    assert np.array_equal(h1, np.maximum(z1, 0.0))
    return out, zs, (z1, z2)


def _assert_inputs_decided(nets, what):
    """The preconditions of part 2, on the float64 oracle alone: encoder pre-activations are odd
    multiples of their grid unit (so exact in fp32 and never zero), and no hidden pre-activation
    lies within fp32 rounding of zero (MASK_EPS of the layer's max |z|)."""
    for name, (_, zs, enc) in nets.items():
        for z, unit, bound in zip(enc, (GRID_Z1_UNIT, GRID_Z2_UNIT), (8.5, 545.0)):
            u = z / unit
            assert np.array_equal(u, np.round(u)), (what, name, unit, "off the grid")
            assert (np.round(u).astype(np.int64) % 2 == 1).all(), (what, name, unit, "even multiple")
            assert np.abs(z).max() <= bound, (what, name, unit)
        for layer, z in enumerate(zs):
            near = np.abs(z) < MASK_EPS * np.abs(z).max()
            assert not near.any(), (what, name, layer, int(near.sum()), "pre-activations within fp32 rounding of 0: "
                                    "take the next data seed")


def _critic_inputs(c, seed):
    S = _setup(c, seed, grid=True)
    rs = np.random.RandomState(1000 + seed)
    idx = rs.randint(0, ROWS, c["B"])
    noise = rs.standard_normal((c["B"], c["A"])).astype(np.float32)
    batch = S["buf"].gather(idx)
    f, p, a = batch[:3]
    nets = {q: _net64(S["critic"], f"{q}.", c["norm"], f, p, a) for q in (("q1", "q2") if c["cdq"] else ("q1",))}
    return S, idx, noise, batch, nets


def _actor_inputs(c, S, seed):
    rs = np.random.RandomState(2000 + seed)
    f = rs.standard_normal((c["B"], c["F"])).astype(np.float32)
    p = grid_particles(rs.standard_normal((c["B"], c["N"], c["D"]))).astype(np.float32)
    nets = {"actor": _net64(S["actor"], "", c["norm"], f, p, actor=True)}
    nets["aq"] = _net64(S["critic"], "q1.", c["norm"], f, p, nets["actor"][0])
    return f, p, nets


@pytest.mark.parametrize("name", list(CASES))
def test_edge_encoder_gradients(name):
    c = _case(name)
    B = c["B"]
    seed_c, seed_a = CASES[name][1]

    # critic step (critic-only: total_it = 1) from zero moments
    S, idx, noise, batch, nets = _critic_inputs(c, seed_c)
    _assert_inputs_decided(nets, (name, "critic"))
    pol, rb = _make(S, rows=ROWS, data=S["data"])
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    L64 = _step64(L, "particles", batch, noise, S["kw"])
    orc.particle_train_step(L, batch, noise)
    pol.train_step(rb, B, indices=idx, noise=noise)
    assert pol._counters() == (1, 1, 0)
    _check(pol.critic_optimizer, L.critic_m, L.critic_v, L64.critic_m, L64.critic_v, 1, (name, "critic"))

    # _actor_learn on B grid rows, a fresh learner in the same grid state
    f, p, nets = _actor_inputs(c, S, seed_a)
    _assert_inputs_decided(nets, (name, "actor"))
    pol, _ = _make(S, rows=ROWS, data=S["data"])
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    L64 = _copy_learner(L, S["kw"])
    with _Float64Oracle():
        orc.particle_actor_learn(L64, f.astype(np.float64), p.astype(np.float64))
    orc.particle_actor_learn(L, f, p)
    pol._actor_learn(f, p)
    assert pol._counters() == (0, 0, 1)
    _check(pol.actor_optimizer, L.actor_m, L.actor_v, L64.actor_m, L64.actor_v, 1, (name, "actor"))


# ------------------------------------------------------------------ part 3
def _create(F, N, D, A):
    from td3_amd.TD3_particles import TD3
    return TD3((Box((F,)), Box((N, D))), Box((A,)), norm="layer", init="none")


def test_particle_dim_17_is_refused():
    from td3_amd._lib import TD3Error
    with pytest.raises(TD3Error, match="particle_dim > 16"):
        _create(7, 16, 17, 3)


def test_input_width_513_is_refused():
    from td3_amd._lib import TD3Error
    with pytest.raises(TD3Error, match="network input width"):
        _create(353, 16, 9, 32)                 # 128 + 353 + 32 = 513 columns (case f352_a32 runs 512)
