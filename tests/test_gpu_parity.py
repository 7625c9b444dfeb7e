"""GPU parity: the HIP path (through the C-ABI) against the CPU oracle and the goldens.

Every test here runs on an MI355X; the oracle (oracle/td3_oracle.py) is the checker.
Tolerances (fp32): forward values / losses rtol 1e-5 (abs floor 1e-6 of
the tensor scale), gradients rtol 1e-4, post-Adam parameters within 1e-6 + 1e-5|x| on
>= 99.9 % of elements and within 2*lr everywhere (sign flips of ~0 gradients).
"""
import numpy as np
import pytest

from helpers import featured_setup_dims, gen, orc, load_golden, featured_setup

pytestmark = pytest.mark.gpu


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


def _rel_to_max(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (np.abs(b).max() + 1e-30))


def _make(S, use_graph=True):
    from td3_amd.TD3_featured import TD3
    from td3_amd.my_replay_buffer import ReplayBuffer_featured
    hp = dict(S["hp"])
    lr = hp.pop("lr", 1e-4)
    pol = TD3(Box((S["sd"],)), Box((S["ad"],)), max_action=S["ma"], norm=S["norm"], lr=lr,
              use_graph=use_graph, init="none", **hp)
    pol.set_weights(S["actor"], S["critic"])
    rb = ReplayBuffer_featured(Box((S["sd"],)), Box((S["ad"],)), max_size=gen.BUFFER_ROWS)
    s, a, s2, r, d = gen.fill_featured_buffer(S["sd"], S["ad"], S["ma"], gen.BUFFER_ROWS, gen.SEED)
    rb.add_batch(s, a, s2, r, d)
    return pol, rb


def _params_close(gpu, ref, lr, what, frac=0.999):
    """SURVEY §8c post-Adam contract: within 1e-6 + 1e-5|x| on >= `frac` of the elements, and within
    2*lr everywhere -- the update of a near-zero gradient whose sign flips between two fp32
    summation orders is +-lr*m/denom ~ +-lr, so the two parameters differ by up to 2*lr (the 0.1 %
    allows for fp32 rounding on top of that bound)."""
    for k in ref:
        g, o = np.asarray(gpu[k], np.float64), np.asarray(ref[k], np.float64)
        err = np.abs(g - o)
        tight = err <= 1e-6 + 1e-5 * np.abs(o)
        assert tight.mean() >= frac or (~tight).sum() <= 2, (what, k, (~tight).sum(), err.max())
        assert err.max() <= 2 * lr * 1.001, (what, k, err.max())


def _load_oracle_state(pol, L):
    pol.set_weights(L.actor, L.critic, L.actor_target, L.critic_target)
    from td3_amd import _lib
    from td3_amd.TD3_featured import _ParamView
    _ParamView(pol, _lib.TD3_ACTOR_ADAM_M, 0).load_state_dict(L.actor_m)
    _ParamView(pol, _lib.TD3_ACTOR_ADAM_V, 0).load_state_dict(L.actor_v)
    _ParamView(pol, _lib.TD3_CRITIC_ADAM_M, 1).load_state_dict(L.critic_m)
    _ParamView(pol, _lib.TD3_CRITIC_ADAM_V, 1).load_state_dict(L.critic_v)
    pol._set_counters(L.total_it, L.critic_step, L.actor_step)


def test_sample_gather_bit_exact():
    S = featured_setup("hc_layer")
    pol, rb = _make(S)
    idx = np.random.RandomState(3).randint(0, gen.BUFFER_ROWS, size=300)
    out = rb.sample(300, indices=idx)
    ref = S["buf"].gather(idx)
    for o, r in zip(out, ref):
        np.testing.assert_array_equal(o.cpu().numpy(), r)


def test_sample_philox_uniform_and_in_range():
    S = featured_setup("hc_layer")
    pol, rb = _make(S)
    counts = np.zeros(gen.BUFFER_ROWS)
    for _ in range(40):
        (s, a, s2, r, nd), idx = rb.sample(1000, return_indices=True)
        ix = idx.cpu().numpy()
        assert ix.min() >= 0 and ix.max() < gen.BUFFER_ROWS
        np.testing.assert_array_equal(s.cpu().numpy(), S["buf"].state[ix].astype(np.float32))
        counts += np.bincount(ix, minlength=gen.BUFFER_ROWS)
    # 40k draws over 1000 bins: chi-square within a generous bound
    e = counts.sum() / counts.size
    chi2 = ((counts - e) ** 2 / e).sum()
    assert chi2 < 1200, chi2


@pytest.mark.parametrize("name", list(gen.FEATURED_CONFIGS))
def test_train_step_teacher_forced(name):
    """Each step starts from the oracle's state; every output of the step is compared."""
    G = load_golden("featured", name)
    S = featured_setup(name)
    pol, rb = _make(S)
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    lr = S["kw"].get("lr", 1e-4)
    for step in range(1, S["steps"] + 1):
        p = f"step{step}"
        idx, noise = G[f"{p}/idx"], G[f"{p}/noise"]
        _load_oracle_state(pol, L)
        rec = orc.featured_train_step(L, S["buf"].gather(idx), noise)
        out = pol.train_step(rb, S["B"], indices=idx, noise=noise, stats=True)
        np.testing.assert_array_equal(out["idx"], idx)
        assert _rel_to_max(out["y"], rec["y"][:, 0]) <= 1e-5, (p, "y")
        assert _rel_to_max(out["q1"], rec["q1"][:, 0]) <= 1e-5, (p, "q1")
        assert _rel_to_max(out["q2"], rec["q2"][:, 0]) <= 1e-5, (p, "q2")
        np.testing.assert_allclose(out["critic_loss"], rec["critic_loss"], rtol=1e-5)
        assert out["actor_step"] == ("actor_loss" in rec)
        if out["actor_step"]:
            np.testing.assert_allclose(out["actor_loss"], rec["actor_loss"], rtol=1e-5, atol=1e-7)
        # the same quantities against the reference goldens directly
        assert _rel_to_max(out["y"], G[f"{p}/y"][:, 0]) <= 2e-5
        _params_close(pol.critic.numpy_dict(), L.critic, lr, (p, "critic"))
        _params_close(pol.critic_target.numpy_dict(), L.critic_target, lr, (p, "critic_target"))
        _params_close(pol.actor.numpy_dict(), L.actor, lr, (p, "actor"))
        _params_close(pol.actor_target.numpy_dict(), L.actor_target, lr, (p, "actor_target"))
        assert pol._counters() == (L.total_it, L.critic_step, L.actor_step)


def test_adam_moments_match_oracle():
    S = featured_setup("hc_layer")
    G = load_golden("featured", "hc_layer")
    pol, rb = _make(S)
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    for step in (1, 2):
        p = f"step{step}"
        orc.featured_train_step(L, S["buf"].gather(G[f"{p}/idx"]), G[f"{p}/noise"])
        pol.train_step(rb, S["B"], indices=G[f"{p}/idx"], noise=G[f"{p}/noise"])
    sd = pol.critic_optimizer.state_dict()
    assert float(sd["state"][0]["step"]) == 2.0
    for i, k in enumerate(L.critic):
        m = sd["state"][i]["exp_avg"].numpy()
        assert _rel_to_max(m, L.critic_m[k]) <= 2e-4, k
    sda = pol.actor_optimizer.state_dict()
    assert float(sda["state"][0]["step"]) == 1.0
    for i, k in enumerate(L.actor):
        assert _rel_to_max(sda["state"][i]["exp_avg"].numpy(), L.actor_m[k]) <= 2e-4, k


@pytest.mark.parametrize("name", ["hc_layer", "hc_none", "pend_layer", "hc_wn"])
def test_free_running_matches_golden(name):
    """Four free-running steps against the reference's own goldens."""
    G = load_golden("featured", name)
    S = featured_setup(name)
    pol, rb = _make(S)
    for step in range(1, S["steps"] + 1):
        p = f"step{step}"
        out = pol.train_step(rb, S["B"], indices=G[f"{p}/idx"], noise=G[f"{p}/noise"], stats=True)
        assert _rel_to_max(out["y"], G[f"{p}/y"][:, 0]) <= 5e-5
        assert _rel_to_max(out["q1"], G[f"{p}/q1"][:, 0]) <= 5e-5
        np.testing.assert_allclose(out["critic_loss"], float(G[f"{p}/critic_loss"]), rtol=5e-5)
        for grp, view, sb in (("actor", pol.actor, 0), ("critic", pol.critic, 500),
                              ("critic_target", pol.critic_target, 500)):
            for i, (k, v) in enumerate(view.numpy_dict().items()):
                st, smp = gen.summarize(v, salt=sb + i)
                ref = G[f"{p}/{grp}/{k}/samples"]
                assert np.abs(smp - ref).max() <= 2.5e-4, (p, grp, k)


def test_graph_equals_eager():
    """Direct launches, graph replays and the auto policy (replays for critic-only steps on an idle
    GPU, direct launches otherwise) run the same kernels: bit-identical parameters."""
    S = featured_setup("hc_layer")
    G = load_golden("featured", "hc_layer")
    outs = []
    for use_graph in (False, True, "auto"):
        pol, rb = _make(S, use_graph=use_graph)
        for step in range(1, 5):
            p = f"step{step}"
            pol.train_step(rb, S["B"], indices=G[f"{p}/idx"], noise=G[f"{p}/noise"])
        outs.append((pol.actor.flat(), pol.critic.flat(), pol.critic_target.flat()))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            np.testing.assert_array_equal(a, b)


def test_select_action_and_eval_q():
    S = featured_setup("hc_layer")
    pol, rb = _make(S)
    rs = np.random.RandomState(0)
    for _ in range(3):
        s = rs.standard_normal(S["sd"]).astype(np.float32)
        a = pol.select_action(s)
        ref = orc.featured_select_action(S["actor"], S["norm"], S["ma"], s)
        assert a.dtype == np.float32 and a.shape == (S["ad"],)
        np.testing.assert_allclose(a, ref, rtol=1e-5, atol=1e-6)
        q = pol.eval_q(s, a)
        q1, _ = orc.featured_q(S["critic"], "q1", S["norm"], s[None], a[None])
        q2, _ = orc.featured_q(S["critic"], "q2", S["norm"], s[None], a[None])
        np.testing.assert_allclose(q[0], q1[0], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(q[1], q2[0], rtol=1e-5, atol=1e-6)


def test_query_kernel_timeout_fails_loudly_and_recovers():
    """when a workgroup of the one-launch query (act_kernel) gives up its in-launch
    layer-1 poll, the launch must not report success with NaN outputs, and its leftover counters
    must not corrupt the next query.  td3_debug_act_fail makes workgroup 0 act as timed out: both
    select_action and eval_q raise, and the next queries are bit-identical to the ones before."""
    from td3_amd import _lib
    S = featured_setup("hc_layer")
    pol, _ = _make(S)
    s = np.random.RandomState(3).standard_normal(S["sd"]).astype(np.float32)
    a0 = pol.select_action(s)
    q0 = pol.eval_q(s, a0)
    for call in (lambda: pol.select_action(s), lambda: pol.eval_q(s, a0)):
        _lib.check(pol._lib.td3_debug_act_fail(pol._h, 1), "td3_debug_act_fail")
        with pytest.raises(_lib.TD3Error, match="timed out"):
            call()
    for _ in range(3):
        np.testing.assert_array_equal(pol.select_action(s), a0)
        q = pol.eval_q(s, a0)
        np.testing.assert_array_equal(q[0], q0[0])
        np.testing.assert_array_equal(q[1], q0[1])


@pytest.mark.parametrize("name", ["hc_layer", "hc_none", "hc_wn"])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 300])
def test_select_action_eval_q_batch_paths(name, n):
    """The query paths of act.hip: n <= 4 rows on the gemv chain (gemv_kernel<1, 2, 4>), up to 256
    padded rows on the GEMM stages with mapped host I/O, more on device buffers and DMA copies
    (kMappedRows) -- actions and both Q values against the oracle row by row; two calls in a
    row reuse the plan's buffers."""
    from td3_amd import _lib
    S = featured_setup(name)
    pol, _ = _make(S)
    rs = np.random.RandomState(n)
    for _ in range(2):
        st = rs.standard_normal((n, S["sd"])).astype(np.float32)
        got = pol.select_action_batch(st)
        assert got.shape == (n, S["ad"])
        qa, qb = pol.eval_q_batch(st, got)
        q1, _ = orc.featured_q(S["critic"], "q1", S["norm"], st, got)
        q2, _ = orc.featured_q(S["critic"], "q2", S["norm"], st, got)
        assert _rel_to_max(qa, q1[:, 0]) <= 1e-5
        assert _rel_to_max(qb, q2[:, 0]) <= 1e-5
        ref = np.stack([orc.featured_select_action(S["actor"], S["norm"], S["ma"], st[i]) for i in range(n)])
        assert _rel_to_max(got, ref) <= 1e-5


@pytest.mark.parametrize("n", [1, 4, 40])
def test_select_action_eval_q_wide_input(n):
    """Humanoid widths (sd 376, ad 17): a layer 0 wider than gemv01 takes (kGemv0K = 64), so
    n <= 4 runs one gemv launch per layer reading the query from mapped host memory."""
    from td3_amd import _lib
    S = featured_setup_dims(376, 17, ma=0.4)
    pol, _ = _make(S)
    st = np.random.RandomState(n).standard_normal((n, 376)).astype(np.float32)
    got = pol.select_action_batch(st)
    ref = np.stack([orc.featured_select_action(S["actor"], S["norm"], S["ma"], x) for x in st])
    assert _rel_to_max(got, ref) <= 1e-5
    q = np.empty(2 * n, np.float32)
    _lib.check(pol._lib.td3_eval_q(pol._h, _lib.fptr(st), _lib.fptr(got), _lib.fptr(q), n), "td3_eval_q")
    for j, qn in enumerate(("q1", "q2")):
        qr, _ = orc.featured_q(S["critic"], qn, S["norm"], st, got)
        assert _rel_to_max(q[j * n:(j + 1) * n], qr[:, 0]) <= 1e-5


def test_weight_norm_init_and_state_dict():
    """norm="weight_normalization": the default init is torch's weight_norm(Linear) (g = ||W||
    per row, v = W), the state dict has the reference's keys and shapes, and set / get round-trips
    (g, v) exactly -- W itself is derived on the device (wn_kernel) and never exported."""
    import torch
    from td3_amd.TD3_featured import TD3
    torch.manual_seed(3)
    pol = TD3(Box((17,)), Box((6,)), norm="weight_normalization")
    sd = pol.actor.state_dict()
    assert list(sd)[:3] == ["linears.0.bias", "linears.0.weight_g", "linears.0.weight_v"]
    assert tuple(sd["linears.0.weight_g"].shape) == (500, 1)
    assert tuple(sd["linears.0.weight_v"].shape) == (500, 17)
    assert not any("lnorms" in k for k in sd)
    v = sd["linears.1.weight_v"].numpy().astype(np.float64)
    np.testing.assert_allclose(sd["linears.1.weight_g"].numpy()[:, 0], np.linalg.norm(v, axis=1), rtol=1e-6)
    rs = np.random.RandomState(0)
    new = {k: rs.standard_normal(t.shape).astype(np.float32) for k, t in sd.items()}
    pol.actor.load_state_dict(new)
    for k, t in pol.actor.state_dict().items():
        np.testing.assert_array_equal(t.numpy(), new[k])
    s = rs.standard_normal(17).astype(np.float32)
    ref = orc.featured_select_action(new, "weight_normalization", 1.0, s)
    assert _rel_to_max(pol.select_action(s), ref) <= 1e-5


def test_foreign_buffer_path():
    """A duck-typed buffer (the reference's own class shape) goes through sample() tensors."""
    S = featured_setup("hc_layer")
    G = load_golden("featured", "hc_layer")
    pol, _ = _make(S)
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    idx, noise = G["step1/idx"], G["step1/noise"]

    class Foreign:
        def sample(self, B):
            import torch
            return tuple(torch.from_numpy(x) for x in S["buf"].gather(idx))

    rec = orc.featured_train_step(L, S["buf"].gather(idx), noise)
    out = pol.train_step(Foreign(), S["B"], noise=noise, stats=True)
    assert _rel_to_max(out["y"], rec["y"][:, 0]) <= 1e-5
    _params_close(pol.critic.numpy_dict(), L.critic, 1e-4, "critic")


@pytest.mark.parametrize("name", ["hc_layer", "hum_layer"])
def test_philox_graph_path_teacher_forced(name):
    """The production path (Philox draws, gather captured in the step graph): the rows and
    noise it drew are read back, the oracle replays the same step, and the results agree.
    HalfCheetah records are sampled inside the first layer (kProGather); Humanoid's 3 KB
    records by the separate gather kernel (learner.h Plan::fuse_gather)."""
    S = featured_setup(name)
    pol, rb = _make(S)
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    seen = set()
    for step in range(1, 5):
        _load_oracle_state(pol, L)
        out = pol.train_step(rb, S["B"], stats=True)
        idx, noise = out["idx"], out["noise"]
        assert idx.min() >= 0 and idx.max() < gen.BUFFER_ROWS
        assert np.isfinite(noise).all() and 0.5 < noise.std() < 1.5
        seen.add(idx.tobytes())
        rec = orc.featured_train_step(L, S["buf"].gather(idx), noise)
        assert _rel_to_max(out["y"], rec["y"][:, 0]) <= 1e-5, step
        assert _rel_to_max(out["q1"], rec["q1"][:, 0]) <= 1e-5, step
        np.testing.assert_allclose(out["critic_loss"], rec["critic_loss"], rtol=1e-5)
        _params_close(pol.critic.numpy_dict(), L.critic, L.lr, (step, "critic"))
        _params_close(pol.actor.numpy_dict(), L.actor, L.lr, (step, "actor"))
        _params_close(pol.critic_target.numpy_dict(), L.critic_target, L.lr, (step, "critic_target"))
    assert len(seen) == 4                                   # a fresh draw every step


def test_philox_noise_is_standard_normal():
    """The target-smoothing noise the step draws (Philox + Box-Muller on the hardware
    transcendentals): N(0, 1) by a Kolmogorov-Smirnov test over 8 steps, a fresh draw per step."""
    from scipy import stats as st
    S = featured_setup("hc_layer")
    pol, rb = _make(S)
    draws = []
    for _ in range(8):
        out = pol.train_step(rb, S["B"], stats=True)
        draws.append(out["noise"].ravel())
    z = np.concatenate(draws).astype(np.float64)
    assert len({d.tobytes() for d in draws}) == len(draws)
    assert abs(z.mean()) < 5.0 / np.sqrt(z.size) and abs(z.std() - 1.0) < 0.05
    assert st.kstest(z, "norm").pvalue > 1e-4


@pytest.mark.parametrize("name,shard", [("hc_layer", "2"), ("hc_layer", "0"), ("hc_wn", "2")])
def test_allreduce_path_single_rank(name, shard, monkeypatch):
    """The data-parallel kernels at nranks = 1 against the oracle, teacher-forced like the fused path:
    grad-only dW, then the sharded step (ncclReduceScatter -> flat Adam on the rank's slice ->
    ncclAllGather -> replicated Polyak; TD3_DP_SHARD=2 forces it at one rank, where the default
    runs the all-reduce form) or RCCL all-reduce + flat Adam + Polyak (0); with weight
    normalization the all-reduced dW feeds wn_kernel."""
    import ctypes as C
    from td3_amd import _lib
    monkeypatch.setenv("TD3_DP_SHARD", shard)
    G = load_golden("featured", name)
    S = featured_setup(name)
    pol, rb = _make(S)
    uid = (C.c_ubyte * 128)()
    _lib.check(pol._lib.td3_comm_unique_id(uid), "td3_comm_unique_id")
    _lib.check(pol._lib.td3_comm_init(pol._h, uid, 1, 0), "td3_comm_init")
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    for step in range(1, 5):
        p = f"step{step}"
        _load_oracle_state(pol, L)
        rec = orc.featured_train_step(L, S["buf"].gather(G[f"{p}/idx"]), G[f"{p}/noise"])
        out = pol.train_step(rb, S["B"], indices=G[f"{p}/idx"], noise=G[f"{p}/noise"], stats=True)
        assert _rel_to_max(out["y"], rec["y"][:, 0]) <= 1e-5, p
        _params_close(pol.critic.numpy_dict(), L.critic, L.lr, (p, "critic"))
        _params_close(pol.actor.numpy_dict(), L.actor, L.lr, (p, "actor"))
        _params_close(pol.critic_target.numpy_dict(), L.critic_target, L.lr, (p, "critic_target"))
        _params_close(pol.actor_target.numpy_dict(), L.actor_target, L.lr, (p, "actor_target"))


def test_overlapped_allreduce_schedule_single_rank(monkeypatch):
    """The overlapped data-parallel schedule (stages.hip add_dw_stage buckets: per-network split-K dW;
    bucket 0's all-reduce and Adam on the comm stream behind dW_1, bucket 1's on the step stream,
    joined back before the next stage) through RCCL at nranks = 1 (TD3_DP_BUCKETS=2 turns it on without peers):
    Humanoid widths at B = 1024, a critic-only and a policy step against the oracle, both Adam moments
    included."""
    import ctypes as C
    from td3_amd import _lib
    monkeypatch.setenv("TD3_DP_BUCKETS", "2")
    S = featured_setup_dims(376, 17, 0.4, "layer", B=1024)
    pol, rb = _make(S)
    uid = (C.c_ubyte * 128)()
    _lib.check(pol._lib.td3_comm_unique_id(uid), "td3_comm_unique_id")
    _lib.check(pol._lib.td3_comm_init(pol._h, uid, 1, 0), "td3_comm_init")
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    rs = np.random.RandomState(17)
    for step in (1, 2):
        idx = rs.randint(0, gen.BUFFER_ROWS, S["B"])
        noise = rs.standard_normal((S["B"], S["ad"])).astype(np.float32)
        _load_oracle_state(pol, L)
        rec = orc.featured_train_step(L, S["buf"].gather(idx), noise)
        out = pol.train_step(rb, S["B"], indices=idx, noise=noise, stats=True)
        assert _rel_to_max(out["y"], rec["y"][:, 0]) <= 1e-5, step
        _params_close(pol.critic.numpy_dict(), L.critic, L.lr, (step, "critic"))
        _params_close(pol.actor.numpy_dict(), L.actor, L.lr, (step, "actor"))
        _params_close(pol.critic_target.numpy_dict(), L.critic_target, L.lr, (step, "critic_target"))
        st = pol.critic_optimizer.state_dict()["state"]
        for i, k in enumerate(L.critic):
            assert _rel_to_max(st[i]["exp_avg"].numpy(), L.critic_m[k]) <= 2e-4, (step, k)
            assert _rel_to_max(st[i]["exp_avg_sq"].numpy(), L.critic_v[k]) <= 4e-4, (step, k)
    ms = (C.c_float * 128)()
    n = C.c_int()
    _lib.check(pol._lib.td3_profile_stages(pol._h, rb.handle, S["B"], 1, ms, 128, C.byref(n)), "profile")
    names = [pol._lib.td3_stage_name(pol._h, i).decode() for i in range(n.value)]
    want = ["C_dw_0", "C_dw_1", "C_0_allreduce", "C_1_allreduce", "C_join"]
    assert [x for x in names if x in want] == want, names


@pytest.mark.parametrize("sd,ad", [(24, 4), (29, 3)])
def test_layer0_widths_teacher_forced(sd, ad):
    """Network inputs of 25..32 columns: the fused layer 0 runs its 16-MFMA K layout (inputs of
    <= 24 columns, every golden config, use 12 MFMAs per tile, kernels_prologues.h l0_koff)."""
    S = featured_setup_dims(sd, ad)
    pol, rb = _make(S)
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    rs = np.random.RandomState(sd)
    for step in (1, 2):
        idx = rs.randint(0, gen.BUFFER_ROWS, S["B"])
        noise = rs.standard_normal((S["B"], ad)).astype(np.float32)
        _load_oracle_state(pol, L)
        rec = orc.featured_train_step(L, S["buf"].gather(idx), noise)
        out = pol.train_step(rb, S["B"], indices=idx, noise=noise, stats=True)
        assert _rel_to_max(out["y"], rec["y"][:, 0]) <= 1e-5, (step, "y")
        assert _rel_to_max(out["q1"], rec["q1"][:, 0]) <= 1e-5, (step, "q1")
        np.testing.assert_allclose(out["critic_loss"], rec["critic_loss"], rtol=1e-5)
        _params_close(pol.critic.numpy_dict(), L.critic, L.lr, (step, "critic"))
        _params_close(pol.actor.numpy_dict(), L.actor, L.lr, (step, "actor"))


@pytest.mark.parametrize("B", [512, 1024])
def test_large_batch_teacher_forced(B):
    """Batches >= 512 switch the wide stages to 128-column GEMM workgroups with the K chunks
    streamed (stages.hip gemm_wn): a critic-only and an actor step against the oracle."""
    S = featured_setup("hc_layer")
    S["B"] = B
    pol, rb = _make(S)
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    rs = np.random.RandomState(B)
    for step in (1, 2):
        idx = rs.randint(0, gen.BUFFER_ROWS, B)
        noise = rs.standard_normal((B, S["ad"])).astype(np.float32)
        _load_oracle_state(pol, L)
        rec = orc.featured_train_step(L, S["buf"].gather(idx), noise)
        out = pol.train_step(rb, B, indices=idx, noise=noise, stats=True)
        assert _rel_to_max(out["y"], rec["y"][:, 0]) <= 1e-5, (step, "y")
        assert _rel_to_max(out["q1"], rec["q1"][:, 0]) <= 1e-5, (step, "q1")
        assert _rel_to_max(out["q2"], rec["q2"][:, 0]) <= 1e-5, (step, "q2")
        np.testing.assert_allclose(out["critic_loss"], rec["critic_loss"], rtol=1e-5)
        if out["actor_step"]:
            np.testing.assert_allclose(out["actor_loss"], rec["actor_loss"], rtol=1e-5, atol=1e-7)
        _params_close(pol.critic.numpy_dict(), L.critic, L.lr, (step, "critic"))
        _params_close(pol.actor.numpy_dict(), L.actor, L.lr, (step, "actor"))
        _params_close(pol.critic_target.numpy_dict(), L.critic_target, L.lr, (step, "critic_target"))


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_one_launch_query_equals_launch_chain(n, monkeypatch):
    """select_action / eval_q of n <= 4 rows as ONE act_kernel launch (in-launch H1 hand-off, head in
    the last-arriving workgroup) against the gemv01 -> gemv -> head chain (TD3_ACT1=0) and the
    oracle.  Layer 0's dot products are summed in another order (4-column partials, butterfly):
    fp32 rounding apart, the same values (SURVEY §8c forward tolerance)."""
    from td3_amd import _lib
    S = featured_setup("hc_layer")
    outs = []
    st = np.random.RandomState(40 + n).standard_normal((n, S["sd"])).astype(np.float32)
    for flag in ("1", "0"):
        monkeypatch.setenv("TD3_ACT1", flag)
        pol, _ = _make(S)
        a = pol.select_action_batch(st)
        q = pol.eval_q_batch(st, a)
        outs.append((a, q[0], q[1]))
    for x, y in zip(outs[0], outs[1]):
        np.testing.assert_allclose(x, y, rtol=1e-5, atol=1e-6)
    ref = np.stack([orc.featured_select_action(S["actor"], S["norm"], S["ma"], x) for x in st])
    assert _rel_to_max(outs[0][0], ref) <= 1e-5


def test_one_launch_query_beside_training():
    """The one-launch query's hand-off while training steps run on the learner stream (critic-only
    steps overlap the acting stream): 60 train + select_action rounds, every action against the
    oracle on the actor the learner holds at that moment."""
    S = featured_setup("hc_layer")
    pol, rb = _make(S)
    rs = np.random.RandomState(5)
    for it in range(60):
        pol.train(rb, 256)
        n = 1 + it % 4
        st = rs.standard_normal((n, S["sd"])).astype(np.float32)
        got = pol.select_action_batch(st) if n > 1 else pol.select_action(st[0])[None]
        actor = pol.actor.numpy_dict()
        ref = np.stack([orc.featured_select_action(actor, S["norm"], S["ma"], x) for x in st])
        assert np.isfinite(got).all()
        assert _rel_to_max(got, ref) <= 1e-5, it
