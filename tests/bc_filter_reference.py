"""numpy reference of the filtered BC term (include/td3.h, "BC on the demonstration rows, Q-filter"; Nair
et al. 2018 §IV-B/C) on top of tests/bc_reference.py and the oracle's public pieces, and the cases the
filter tests share.

    n_d    = n_demo of the step if demo_rows, else B
    keep_r = r < n_d and (not q_filter or Q1(s_r, a_r) > Q1(s_r, pi_r))     float32 compare, strict
             Q1(s, a): the step's critic phase (rec["q1"], the critic before the step's update)
             Q1(s, pi): the actor phase (rec["actor_q1"], the critic after it)
    dL/dpi = lambda dQ1/da + keep_r c (pi - a),   c = (float)(2.0 / ((double)n_d * A))
    bc_loss = sum_r keep_r sum_o (pi - a)^2 / (n_d A)      (0 when n_d = 0)
"""
from __future__ import annotations

import numpy as np

import bc_reference as bcr
from helpers import featured_setup, featured_setup_dims, gen, orc

f32 = np.float32
MIN_GAP = 1e-4             # min |Q1sa - Q1pi| over the candidates, of max |Q1|: ten forward tolerances (1e-5 a side)
MIN_ROWS, MIN_FRACTION = 3, 0.10      # kept and dropped candidates of a filtered case: at least this many each

MODES = {"demo": (1, 0), "filter": (0, 1), "both": (1, 1)}      # (demo_rows, q_filter)

# The teacher-forced mixed cases: a golden configuration's name or an edge shape of bcr.EDGES (its alpha
# with it).  hc_layer_b100: the narrow head, fused sample dims; hum_layer: A = 17, the LDS-staged wide
# head, the split gather; the edges: A = 1 at a ragged B, the wide head at B = 100, norm None at B = 257
# (A = 9: the head's second block of outputs holds one), B = 1000 (more than one trip of lambda's sum).
TF_CASES = ["hc_layer_b100", "hum_layer", (5, 1, 2.0, "layer", 33), (40, 17, 2.0, "layer", 100),
            (11, 9, 2.0, None, 257), (17, 6, 1.0, "layer", 1000)]
EDGE_N_DEMO_CASES = ["hc_layer_b100", (40, 17, 2.0, "layer", 100)]     # one narrow, one wide: n_demo 0, 1, B too
# alpha of a case: the one tests/bc_reference.py gives it, except where the masked BC term then misses
# bcr.MIN_SHARE.  hum_layer at 2.5: 9.0 % with the filter over all rows (81 of 128 kept), 9.1 % at n_demo 127;
# at 1.0 every mode carries it (tests/test_bc_filter_reference.py prints the shares).
ALPHA = {"hum_layer": 1.0}


def case_alpha(case):
    if case in ALPHA:
        return ALPHA[case]
    return dict(bcr.CASES)[case] if isinstance(case, str) else {e[:5]: e[5] for e in bcr.EDGES}[case]


def case_id(case):
    return case if isinstance(case, str) else "sd%d_ad%d_B%d" % (case[0], case[1], case[4])


_SETUPS = {}


def case_setup(case):
    """(setup, golden name or None, alpha) of a TF_CASES entry; setups are built once per case."""
    if case not in _SETUPS:
        if isinstance(case, str):
            _SETUPS[case] = (featured_setup(case), case, case_alpha(case))
        else:
            _SETUPS[case] = (featured_setup_dims(*case), None, case_alpha(case))
    return _SETUPS[case]


def tf_params():
    """[(case, n_demo, mode)] of the teacher-forced mixed steps: n_demo in {B // 2, B - 1} for the two modes
    that read it (plus 0, 1, B on EDGE_N_DEMO_CASES); the filter alone has n_d = B whatever n_demo is, so it
    runs once per case, at B // 2."""
    out = []
    for case in TF_CASES:
        B = gen.FEATURED_CONFIGS[case][4] if isinstance(case, str) else case[4]
        nds = [B // 2, B - 1] + ([0, 1, B] if case in EDGE_N_DEMO_CASES else [])
        out += [(case, nd, mode) for mode in ("demo", "both") for nd in nds]
        out.append((case, B // 2, "filter"))
    return out


def tf_id(p):
    return "%s-nd%d-%s" % (case_id(p[0]), p[1], p[2])


def ring_indices(idx, n_demo):
    """The injected indices of a mixed step whose batch is the case's own: the demo ring holds the case's
    buffer in order, the online ring holds it reversed, so batch row r reads buffer row idx[r] from
    either -- and a row taken from the wrong ring is another transition."""
    idx = np.asarray(idx, np.int64)
    out = idx.copy()
    out[n_demo:] = gen.BUFFER_ROWS - 1 - idx[n_demo:]
    return out


def n_candidates(B, demo_rows, n_demo):
    return int(n_demo) if demo_rows and n_demo is not None else int(B)


def filtered_actor_grads(L, s, a, alpha, q1sa, demo_rows, q_filter, n_demo=None, record=None, masks=None):
    """``bcr.bc_actor_grads`` with the row mask; ``q1sa``: [B, 1] Q1(s, a) of the step's critic phase.
    Records what that function records (bc_loss and gpi_bc masked) and keep, n_d, kept."""
    rec = record if record is not None else {}
    B, A = a.shape
    masks = masks or {}
    n_d = n_candidates(B, demo_rows, n_demo)
    pi, (alin, aln, acache, t) = orc.featured_actor(L.actor, L.norm, L.max_action, s)
    aq1, (qlin, qln, qcache) = orc.featured_q(L.critic, "q1", L.norm, s, pi)
    if "actor" in masks:
        acache["mask"] = masks["actor"]
    if "aq" in masks:
        qcache["mask"] = masks["aq"]
    qabs = f32(np.mean(np.abs(aq1), dtype=np.float64))
    with np.errstate(divide="ignore"):
        lam = f32(alpha) / qabs
    keep = np.arange(B) < n_d
    if q_filter:
        with np.errstate(invalid="ignore"):
            keep &= np.asarray(q1sa, f32).reshape(B) > aq1.astype(f32).reshape(B)      # NaN on either side: dropped
    d = (pi - a.astype(f32)).astype(f32)
    se = np.sum(d.astype(np.float64) ** 2, axis=1)
    bc_loss = float(np.sum(se[keep]) / (n_d * A)) if n_d else 0.0
    actor_loss = -float(np.mean(aq1, dtype=np.float64))
    gq = np.full((B, 1), -1.0 / B, dtype=f32)
    _, gx = orc.mlp_backward(qlin, qln, qcache, gq)
    gpi_q = (lam * gx[:, s.shape[1]:]).astype(f32)
    gpi_bc = np.zeros_like(d)
    if n_d:
        c = f32(2.0 / (float(n_d) * A))
        gpi_bc[keep] = (c * d[keep]).astype(f32)
    gpi = (gpi_q + gpi_bc).astype(f32)
    gz = (gpi * f32(L.max_action)) * (f32(1) - t * t)
    ag, _ = orc.mlp_backward(alin, aln, acache, gz.astype(f32))
    agrads = orc.pack_mlp_grads("", ag, L.norm, P=L.actor)
    rec.update(pi=pi, actor_q1=aq1, actor_loss=actor_loss, q_abs_mean=float(qabs), bc_loss=bc_loss,
               bc_actor_loss=float(lam) * actor_loss + bc_loss, gpi_q=gpi_q, gpi_bc=gpi_bc, actor_grads=agrads,
               keep=keep, n_d=n_d, kept=int(keep.sum()))
    rec["lambda"] = float(lam)
    return agrads


def filtered_featured_step(L, batch, noise, alpha, demo_rows, q_filter, n_demo=None, w=None, masks=None):
    """``bcr.bc_featured_step`` with the filtered actor loss.  The critic phase is that function's own: it
    is called with the learner's policy_freq moved out of reach, so it stops behind the critic's Adam step,
    and the actor phase (filtered gradients, Adam, Polyak) follows here as it does there."""
    s, a = batch[0], batch[1]
    freq = L.policy_freq
    actor_phase = (L.total_it + 1) % freq == 0
    L.policy_freq = L.total_it + 2
    try:
        rec = bcr.bc_featured_step(L, batch, noise, alpha, w=w, masks=masks)
    finally:
        L.policy_freq = freq
    if actor_phase:
        if alpha:
            g = filtered_actor_grads(L, s, a, alpha, rec["q1"], demo_rows, q_filter, n_demo, rec, masks)
        else:
            g = orc.featured_actor_grads(L, s, rec, masks)
        L.adam_actor(g)
        L.polyak()
    return rec


def gap(rec):
    """min over the candidate rows of |Q1sa - Q1pi|, as a share of max |Q1| over both sides (all rows)."""
    qa, qp = rec["q1"].astype(np.float64)[:, 0], rec["actor_q1"].astype(np.float64)[:, 0]
    cand = np.arange(qa.size) < rec["n_d"]
    if not cand.any():
        return np.inf
    return float(np.min(np.abs(qa - qp)[cand]) / max(np.abs(qa).max(), np.abs(qp).max()))


def check_case(rec, n_demo, q_filter, what):
    """The conditions that make a GPU comparison of this actor step meaningful (tests/test_bc_filter_reference.py
    states them); prints the figures, returns them."""
    n_d, kept = rec["n_d"], rec["kept"]
    g = gap(rec)
    sq, sb = bcr.term_shares(rec)
    print(f"{what}: n_d {n_d}, kept {kept}, gap {g:.2e} of max|Q1|, Q term {sq:.3f}, BC term {sb:.3f} of |dL/dpi|")
    if q_filter:
        assert g >= MIN_GAP, (what, g)
        if n_d > 1:
            dropped = n_d - kept
            assert min(kept, dropped) >= max(MIN_ROWS, MIN_FRACTION * n_d), (what, n_d, kept)
    assert sq >= bcr.MIN_SHARE, (what, sq, sb)
    # (the n_demo edges: with n_d = 0 no row is a candidate, and with n_d = 1 the filter may drop the one
    # there is; the step then has no BC term by definition, whatever alpha)
    if kept or n_d > 1:
        assert sb >= bcr.MIN_SHARE, (what, sq, sb)
    return g, sq, sb
