"""The numpy reference of the filtered BC term (tests/bc_filter_reference.py) on the CPU: with both
switches off it is tests/bc_reference.py exactly, and every case the GPU tests use is one whose comparison
means something:

* the filter is exactly decided: over the candidate rows min |Q1sa - Q1pi| >= 1e-4 max |Q1|.  The forward
  tolerance is 1e-5 of the max on each side, so a smaller gap could flip a row between the oracle and the
  device, and a flip is a discrete change of the gradient, not a rounding difference;
* the filter is not decoration: among the candidates both the kept and the dropped rows are at least 10 %
  and at least 3 rows (the n_demo edges 0 and 1 are exempt);
* bcr.MIN_SHARE holds for both terms of dL/dpi.
"""
import copy

import numpy as np
import pytest

import bc_filter_reference as bfr
import bc_reference as bcr
from helpers import featured_setup, featured_setup_dims, orc


def _two_steps(S, name, alpha, demo_rows, q_filter, n_demo):
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    for idx, noise in bcr.case_steps(S, name):
        rec = bfr.filtered_featured_step(L, S["buf"].gather(idx), noise, alpha, demo_rows, q_filter, n_demo)
    return L, rec


@pytest.mark.parametrize("case", ["hc_layer_b100", "hc_wn", (11, 9, 2.0, None, 257)], ids=bfr.case_id)
def test_switches_off_is_the_bc_reference(case):
    if isinstance(case, str):
        S, name, alpha = featured_setup(case), case, 2.5
    else:
        S, name, alpha = featured_setup_dims(*case), None, 2.5
    La = orc.Learner(S["actor"], S["critic"], **S["kw"])
    for idx, noise in bcr.case_steps(S, name):
        ra = bcr.bc_featured_step(La, S["buf"].gather(idx), noise, alpha)
    # off outright, and demo_rows on a step that draws from one ring (n_demo None): n_d = B, every row kept
    for demo_rows in (0, 1):
        Lb, rb = _two_steps(S, name, alpha, demo_rows, 0, None)
        assert rb["n_d"] == rb["kept"] == S["B"] and rb["keep"].all()
        for k in ("y", "q1", "q2", "pi", "actor_q1", "gpi_q", "gpi_bc"):
            np.testing.assert_array_equal(ra[k], rb[k], err_msg=k)
        for k in ("critic_loss", "actor_loss", "lambda", "q_abs_mean", "bc_loss", "bc_actor_loss"):
            assert ra[k] == rb[k], k
        for grp in ("actor", "critic", "actor_target", "critic_target", "actor_m", "actor_v", "critic_m", "critic_v"):
            for k, v in getattr(La, grp).items():
                np.testing.assert_array_equal(v, getattr(Lb, grp)[k], err_msg=f"{grp} {k}")
    # and with alpha = 0 the switches change nothing: the oracle's own step
    Lc = orc.Learner(S["actor"], S["critic"], **S["kw"])
    Ld = copy.deepcopy(Lc)
    for idx, noise in bcr.case_steps(S, name):
        orc.featured_train_step(Lc, S["buf"].gather(idx), noise)
        bfr.filtered_featured_step(Ld, S["buf"].gather(idx), noise, 0.0, 1, 1, 3)
    for grp in ("actor", "actor_m", "critic", "actor_target"):
        for k, v in getattr(Lc, grp).items():
            np.testing.assert_array_equal(v, getattr(Ld, grp)[k], err_msg=f"alpha 0: {grp} {k}")


def test_mask_and_scale_by_hand():
    """The definition on a step small enough to read: rows past n_d and rows the critic rates below the
    policy's carry no BC term, the others 2/(n_d A) (pi - a); bc_loss over n_d A."""
    S = featured_setup_dims(5, 1, 2.0, "layer", 33)
    _, rec = _two_steps(S, None, 2.5, 1, 1, 16)
    B, A = 33, 1
    qa, qp = rec["q1"][:, 0], rec["actor_q1"][:, 0]
    keep = (np.arange(B) < 16) & (qa > qp)
    np.testing.assert_array_equal(rec["keep"], keep)
    assert rec["n_d"] == 16 and rec["kept"] == keep.sum()
    d = rec["pi"] - S["buf"].gather(bcr.case_steps(S)[1][0])[1]
    np.testing.assert_array_equal(rec["gpi_bc"][~keep], 0)
    np.testing.assert_array_equal(rec["gpi_bc"][keep], (np.float32(2.0 / (16 * A)) * d[keep]).astype(np.float32))
    np.testing.assert_allclose(rec["bc_loss"], float(np.sum(d[keep].astype(np.float64) ** 2)) / (16 * A), rtol=1e-12)
    # a NaN on either side of the compare drops the row
    L = orc.Learner(S["actor"], S["critic"], **S["kw"])
    (s, a, _, _, _) = S["buf"].gather(bcr.case_steps(S)[1][0])
    q1sa = np.full((B, 1), np.inf, np.float32)
    q1sa[3] = np.nan
    r2 = {}
    bfr.filtered_actor_grads(L, s, a, 2.5, q1sa, 0, 1, None, r2)
    assert not r2["keep"][3] and r2["kept"] == B - 1
    # n_d = 0: lambda-scaled TD3
    _, r0 = _two_steps(S, None, 2.5, 1, 0, 0)
    assert r0["n_d"] == r0["kept"] == 0 and r0["bc_loss"] == 0.0 and not r0["gpi_bc"].any()


@pytest.mark.parametrize("p", bfr.tf_params(), ids=bfr.tf_id)
def test_gpu_mixed_cases_qualify(p):
    case, n_demo, mode = p
    S, name, alpha = bfr.case_setup(case)
    demo_rows, q_filter = bfr.MODES[mode]
    _, rec = _two_steps(S, name, alpha, demo_rows, q_filter, n_demo)
    assert rec["n_d"] == (n_demo if demo_rows else S["B"])
    bfr.check_case(rec, n_demo, q_filter, bfr.tf_id(p))


@pytest.mark.parametrize("case", [c for c, _ in bcr.CASES] + [e[:5] for e in bcr.EDGES], ids=bfr.case_id)
def test_every_bc_case_qualifies_with_the_filter_alone(case):
    """The filter over all B rows on the 15 cases of tests/bc_reference.py (the other step kinds and the
    launch variants of the GPU tests draw from them)."""
    S, name, alpha = bfr.case_setup(case)
    _, rec = _two_steps(S, name, alpha, 0, 1, None)
    bfr.check_case(rec, None, 1, bfr.case_id(case))
