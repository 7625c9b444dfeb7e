"""CPU checks of the particle learner's prioritized step: the weighted reference step
(per_particles_reference.py) against the golden-pinned oracle, its |TD error| against the featured
definition, and the entry point at the C-ABI boundary (exported, bound as the header declares it, its
argument checks made before the handle is looked at)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import per_particles_reference as ppr
import per_reference as per
from helpers import gen, orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "td3_train_step_prioritized_particles"


@pytest.mark.parametrize("name", ppr.CASES)
def test_unit_weights_reproduce_the_oracle_bit_for_bit(name):
    """w = 1 over two steps (critic-only, then the actor phase): every output and every parameter,
    moment and counter equals orc.particle_train_step's."""
    S = ppr.setup(name)
    La = orc.Learner(S["actor"], S["critic"], **S["kw"])
    Lb = orc.Learner(S["actor"], S["critic"], **S["kw"])
    rs = np.random.RandomState(3)
    for step in (1, 2):
        idx = rs.randint(0, gen.BUFFER_ROWS, size=S["B"])
        noise = rs.standard_normal((S["B"], S["A"])).astype(np.float32)
        batch = S["buf"].gather(idx)
        ra = ppr.weighted_particle_step(La, batch, noise, np.ones(S["B"], np.float32))
        rb = orc.particle_train_step(Lb, batch, noise)
        for k in ("y", "q1", "q2", "actor_q1"):
            assert (k in ra) == (k in rb)
            if k in rb:
                np.testing.assert_array_equal(ra[k], rb[k], err_msg=f"{step} {k}")
        assert ra["critic_loss"] == rb["critic_loss"]
        assert ra.get("actor_loss") == rb.get("actor_loss") and ("actor_loss" in rb) == (step == 2)
        for g in ("actor", "critic", "actor_target", "critic_target", "actor_m", "actor_v", "critic_m", "critic_v"):
            for k, v in getattr(Lb, g).items():
                np.testing.assert_array_equal(getattr(La, g)[k], v, err_msg=f"{step} {g} {k}")
        assert (La.total_it, La.critic_step, La.actor_step) == (Lb.total_it, Lb.critic_step, Lb.actor_step)


def test_weights_change_the_step():
    """The teacher-forced inputs discriminate: the smallest weight is <= 0.35, the weighted loss is
    well below the unweighted one and the critic's first moments differ."""
    for name in ppr.CASES:
        S, p, u, noise = ppr.step_case(name, 1)
        idx = per.draw(p, u)
        w = per.weights(p, idx, gen.BUFFER_ROWS, 1.0)
        assert w.min() <= 0.35 and w.max() == 1.0
        La = orc.Learner(S["actor"], S["critic"], **S["kw"])
        Lb = orc.Learner(S["actor"], S["critic"], **S["kw"])
        ra = ppr.weighted_particle_step(La, S["buf"].gather(idx), noise, w)
        rb = orc.particle_train_step(Lb, S["buf"].gather(idx), noise)
        assert ra["critic_loss"] < 0.8 * rb["critic_loss"]
        k = "q1.linears.3.weight"
        assert np.abs(La.critic_m[k] - Lb.critic_m[k]).max() > 0.1 * np.abs(Lb.critic_m[k]).max()


def test_td_abs_is_the_featured_definition_for_one_output():
    """A = 1 with CDQ: 1/(J*A) sum_j sum_o |Q_j - y| is the featured step's 0.5 (|Q1 - y| + |Q2 - y|)."""
    rs = np.random.RandomState(0)
    q1, q2, y = (rs.standard_normal((64, 1)).astype(np.float32) for _ in range(3))
    ref = 0.5 * (np.abs((q1 - y).astype(np.float64)) + np.abs((q2 - y).astype(np.float64)))[:, 0]
    np.testing.assert_array_equal(ppr.td_abs_rows([q1, q2], y), ref)
    # and the general form: the mean over both critics' A outputs
    q1, q2, y = (rs.standard_normal((8, 3)).astype(np.float32) for _ in range(3))
    ref = np.concatenate([np.abs(q1 - y), np.abs(q2 - y)], axis=1).astype(np.float64).mean(axis=1)
    np.testing.assert_allclose(ppr.td_abs_rows([q1, q2], y), ref, rtol=1e-12)
    np.testing.assert_allclose(ppr.td_abs_rows([q1], y), np.abs(q1 - y).astype(np.float64).mean(axis=1), rtol=1e-12)


@pytest.fixture(scope="module")
def lib():
    from td3_amd.build import build_library
    build_library()
    from td3_amd import _lib
    return _lib.load()


def _header_args(name):
    txt = open(os.path.join(ROOT, "include", "td3.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint %s\((.*?)\);" % name, txt, flags=re.S)
    assert m, f"{name} is not declared in include/td3.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_entry_exported_and_bound_as_the_header_declares(lib):
    from td3_amd import _lib
    assert hasattr(lib, ENTRY), f"{ENTRY} not exported"
    assert ENTRY in _lib.SIGNATURES, f"{ENTRY} not bound in td3_amd/_lib.py"
    res, args = _lib.SIGNATURES[ENTRY]
    assert getattr(lib, ENTRY).restype is res is C.c_int
    assert getattr(lib, ENTRY).argtypes == args
    assert _header_args(ENTRY) == ["td3_handle* h", "rb_handle* rb", "int batch", "double beta", "void* stream",
                                   "const float* inject_u", "const float* inject_noise", "td3_step_stats* stats",
                                   "td3_per_stats* per"]
    assert args == [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, _lib._F, _lib._F,
                    C.POINTER(_lib.td3_step_stats), C.POINTER(_lib.td3_per_stats)]
    # the same argument list as the featured entry, which the header declares too
    assert args == _lib.SIGNATURES["td3_train_step_prioritized"][1]
    assert [a.split()[-1] for a in _header_args("td3_train_step_prioritized")] == \
        [a.split()[-1] for a in _header_args(ENTRY)]


def test_entry_refuses_null_handles(lib):
    assert getattr(lib, ENTRY)(None, None, 8, 0.4, None, None, None, None, None) == -1
    assert b"null handle" in lib.td3_last_error()


def test_header_points_particle_learners_to_the_entry():
    txt = open(os.path.join(ROOT, "include", "td3.h")).read()
    assert "takes no importance weights" not in txt
    src = open(os.path.join(ROOT, "td3_amd", "csrc", "step.hip")).read()
    assert "takes no importance weights" not in src
    assert re.search(r"particle learner \(use %s\)" % ENTRY, src)
