"""Path selection of the batched solvers without a GPU: the host-only plan (dff_debug_msm_batch_plan, the function that
dff_msm_dirichlet_solve, dff_sym_eig_topk and dff_msm_propagate go through) against tests/golden/batch_plan_table.json -- the
three selection rules as each call stated them on its own, written down by tests/golden/make_batch_plan_table.py -- and the
properties the rules promise.  One GPU test holds the plan to what the forced paths compute.

A problem's SIZE is what its kernel compares with a launch's lo .. hi: K_p, or for the Dirichlet solver the interior count,
which the host does not know: any of 0 .. K_p - 1.  Two rules of the Dirichlet solver are recorded as they are today:
  * at knob 0 its LDS launch exists whatever the state counts, also when every K_p lies above the limit (such a problem may
    still have few interior states);
  * at knob 0 its blocked launch exists as soon as a K_p exceeds the limit, one state early: with max K_p = limit + 1 no
    interior count can reach it."""
import json
import os

import numpy as np
import pytest

from dff_amd import binding
from support import dev, same_bits, to_dev  # noqa: F401  (dev)

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
with open(os.path.join(ROOT, "tests", "golden", "batch_plan_table.json")) as f:
    TABLE = json.load(f)
LDS_MAX = 160 * 1024
CALLS = ("dirichlet", "eig", "propagate")
KNOB = {"dirichlet": binding.debug_msm_dirichlet_path, "eig": binding.debug_sym_eig_path,
        "propagate": binding.debug_msm_propagate_path}
LIMIT = {"dirichlet": binding.msm_dirichlet_lds_limit, "eig": binding.sym_eig_lds_limit,
         "propagate": binding.msm_propagate_lds_limit}


def plans(call):
    """(record, the library's plan or the message of its refusal) of every record of `call`, each under the record's knob"""
    try:
        for r in TABLE["records"]:
            if r["call"] == call:
                KNOB[call](r["knob"])
                try:
                    yield r, binding.msm_batch_plan(call, r["ks"], TABLE["kmax"])
                except ValueError as e:
                    yield r, str(e)
    finally:
        KNOB[call](0)


def sizes(call, ks):
    """every size a problem of the batch may have"""
    return {n for k in ks for n in range(k)} if call == "dirichlet" else set(ks)


def test_the_table_holds_the_cases_the_rules_name():
    assert {c: LIMIT[c]() for c in CALLS} == TABLE["limits"]
    for call in CALLS:
        L = TABLE["limits"][call]
        recs = [r for r in TABLE["records"] if r["call"] == call]
        knobs = sorted({r["knob"] for r in recs})
        assert knobs == ([0, 1, 2, 3, 4] if call == "dirichlet" else [0, 1, 2])
        for knob in knobs:
            ks = [r["ks"] for r in recs if r["knob"] == knob]
            single = {k[0] for k in ks if len(k) == 1}
            assert single == {1, L, L + 1, 1024} | ({L + 2} if call == "dirichlet" else set())
            top = L + (call == "dirichlet")                        # the largest K_p the LDS path can take
            assert any(len(k) > 1 and max(k) <= top for k in ks) and any(len(k) > 1 and min(k) > top for k in ks)
            assert any(len(k) == 2 and min(k) <= top < max(k) for k in ks)
            assert any(len(k) > 2 and k[-1] <= top and all(v > top for v in k[:-1]) for k in ks)
        assert any("refused" in r for r in recs) and any("launches" in r for r in recs)


@pytest.mark.parametrize("call", CALLS)
def test_plan_is_what_the_call_selected(call):
    """launched / path / lo / hi / sizing argument of both launches of every record; the refusal's words where the call refused"""
    n = 0
    for r, got in plans(call):
        if "refused" in r:
            assert isinstance(got, str) and r["refused"] in got, (r, got)
            continue
        assert not isinstance(got, str), (r, got)
        for want, l in zip(r["launches"], got):
            if want is None:
                assert l == dict(launched=0, path=0, lo=0, hi=0, sized_for=0, lds_bytes=0), (r, l)
                continue
            assert (l["launched"], l["path"], l["lo"], l["hi"]) == (1, want[0], want[1], want[2]), (r, l)
            assert want[3] is None or l["sized_for"] == want[3], (r, l)
            n += 1
    assert n > 20


@pytest.mark.parametrize("call", CALLS)
def test_the_two_launches_split_the_batch(call):
    """Disjoint ranges that together take every size a live problem may have; no launch without a problem it may take, but for
    the Dirichlet solver's early blocked launch; never more LDS than a CU has."""
    L = TABLE["limits"][call]
    for r, got in plans(call):
        if isinstance(got, str):
            continue
        live = [l for l in got if l["launched"]]
        assert live and all(0 < l["lds_bytes"] <= LDS_MAX and l["lo"] <= l["hi"] for l in live), (r, got)
        if len(live) == 2:
            assert got[0]["path"] == 1 and got[1]["path"] == 2 and got[0]["hi"] < got[1]["lo"], (r, got)
        may = sizes(call, r["ks"])
        assert all(any(l["lo"] <= n <= l["hi"] for l in live) for n in may), (r, got)
        for l in live:
            early = call == "dirichlet" and r["knob"] == 0 and l["path"] == 2 and max(r["ks"]) == L + 1
            assert any(l["lo"] <= n <= l["hi"] for n in may) != early, (r, l)
        if call == "dirichlet" and r["knob"] == 0:
            assert got[0]["launched"] and (got[0]["lo"], got[0]["hi"]) == (0, L), (r, got)


# ---- the plan against the forced paths, on the GPU
def _symmetric(rng, K):
    a = rng.random((K, K)) + 0.05
    return a + a.T


def _solver(call, rng, ks, Kmax):
    """a batch of the call's problems -> run(idx): the outputs, as host arrays, of a call on the problems idx alone, under the
    knob as it stands"""
    P = len(ks)
    mats = np.zeros((P, Kmax, Kmax))
    for p, K in enumerate(ks):
        m = _symmetric(rng, K)
        mats[p].reshape(-1)[:K * K] = (m / m.sum(1, keepdims=True) if call == "propagate" else m).reshape(-1)
    w0, obs = rng.random((P, 2, Kmax)), rng.random((P, 3, Kmax))
    role = np.zeros((P, Kmax), np.int32)
    role[:, 0] = 1                                                 # one boundary state: K_p - 1 interior ones
    g, s = rng.random((P, Kmax)), np.ones((P, Kmax))

    def run(idx):
        k, a = [ks[p] for p in idx], to_dev(mats[idx])
        if call == "eig":
            res = binding.sym_eig_topk(a, k, 3, vectors=True)
        elif call == "propagate":
            res = binding.msm_propagate(a, None, k, to_dev(w0[idx]), to_dev(obs[idx]), 4, want_last=True)
        else:
            res = binding.msm_dirichlet_solve(a, k, to_dev(role[idx]), to_dev(g[idx]), to_dev(s[idx]))
        return [t.cpu().numpy() for t in res]
    return run


@pytest.mark.gpu
@pytest.mark.parametrize("call", CALLS)
def test_each_problem_gets_the_bits_of_the_path_the_plan_names(dev, call):
    """One mixed batch at knob 0, ks = {2, L, L + 1}: every output of problem p equals, bit for bit, what the call computes
    with the path forced that the plan names for p's size -- on the problems of that path alone, since a forced LDS path
    refuses a batch that holds a larger one (a problem's bits do not depend on its batch)."""
    L = LIMIT[call]()
    ks, Kmax = [2, L, L + 1], L + 1
    plan = binding.msm_batch_plan(call, ks, Kmax)
    named = []
    for K in ks:
        size = K - 1 if call == "dirichlet" else K
        paths = [l["path"] for l in plan if l["launched"] and l["lo"] <= size <= l["hi"]]
        assert len(paths) == 1, (K, plan)
        named.append(paths[0])
    assert named == ([1, 1, 1] if call == "dirichlet" else [1, 1, 2])
    run = _solver(call, np.random.default_rng(5), ks, Kmax)
    by_size = run([0, 1, 2])
    try:
        for path in sorted(set(named)):
            idx = [p for p in range(3) if named[p] == path]
            KNOB[call](path)
            forced = run(idx)
            for got, want in zip(by_size, forced):
                for j, p in enumerate(idx):
                    assert same_bits(got[p], want[j]), (call, p, ks[p], path)
    finally:
        KNOB[call](0)
    for p in range(3):
        assert not np.isnan(by_size[0][p][..., :1]).any(), (call, p)
