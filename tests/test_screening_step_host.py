"""The recorded oracle steps that tests/test_hip_screening_step.py holds `step_screening` to are fit for it (no GPU):
no decision of the oracle sits near a tie at any step used, the configurations do what they were chosen for, and
the helper's save and restore of the oracle's state reproduces a step bit for bit."""
import numpy as np
import pytest

import screening_step_model as M

CASES = ["C1", "C2", "C3", "C5", "C7"]


@pytest.fixture(params=CASES)
def recorded(request):
    return (request.param,) + M.record(request.param)


def test_iteration_counts(recorded):
    name, p, rec, iterations = recorded
    want = M.ITERATIONS[name]
    assert iterations[:len(want)] == want
    assert set(p.steps) == set(rec) and max(p.steps) < len(iterations)
    for k, r in rec.items():
        assert r["whole"]["iterations"] == iterations[k] == len(r["whole"]["errors"])
        # tolerance 1e300: exactly one iteration, from the same state
        assert r["single"]["iterations"] == 1 and len(r["single"]["errors"]) == 1
        assert r["single"]["errors"][0] == r["whole"]["errors"][0]


def test_no_convergence_decision_is_marginal(recorded):
    name, p, rec, _ = recorded
    worst = np.inf
    for k, r in rec.items():
        errors = np.array(r["whole"]["errors"])
        margin = np.abs(errors - M.TOLERANCE) / M.TOLERANCE
        assert margin.min() >= M.MARGIN_ERROR, (name, k, margin.min())
        # ... and they say what the loop did: only the last one is below the tolerance
        assert np.all(errors[:-1] >= M.TOLERANCE) and errors[-1] < M.TOLERANCE
        worst = min(worst, margin.min())
    print(f"{name}: smallest |e_i - tol| / tol over the steps used = {worst:.1e}")


def test_no_retry_decision_is_marginal(recorded):
    name, p, rec, _ = recorded
    worst = np.inf
    for k, r in rec.items():
        for take in ("whole", "single"):
            for a in r[take]["attempts"]:
                assert (a["margin"] < -M.MARGIN_DISC) if a["failed"] else (a["margin"] > M.MARGIN_DISC), (name, k, take, a)
                worst = min(worst, abs(a["margin"]))
            # one accepted update per screening iteration, the failed ones on top
            assert sum(not a["failed"] for a in r[take]["attempts"]) == r[take]["iterations"]
    print(f"{name}: smallest |disc| / (b^2 + 4 |z|^2 |w|^2) over the updates tried = {worst:.1e}")


def test_every_step_really_screens(recorded):
    name, p, rec, _ = recorded
    for k, r in rec.items():
        for take in ("whole", "single"):
            assert np.abs(r[take]["A_induced"]).max() > M.MIN_A_INDUCED, (name, k, take)
    starts = [np.abs(r["before"]["A_induced"]).max() for r in rec.values()]
    assert max(starts) > M.MIN_A_INDUCED  # a step that starts from a non-zero A_induced ...
    if name != "C5":
        assert min(starts) == 0.0         # ... and one that starts from zero


def test_save_and_restore_reproduce_a_step_bit_for_bit(recorded):
    name, p, rec, _ = recorded
    for k, r in rec.items():
        a, b = r["whole"], r["again"]
        for key in ("psi", "mu", "js", "jn", "A_induced", "mu_boundary", "A_applied"):
            assert np.array_equal(a[key], b[key]), (name, k, key)
        assert a["dt"] == b["dt"] and a["errors"] == b["errors"] and a["attempts"] == b["attempts"]


def test_what_each_configuration_is_for():
    sizes = {name: (len(M.record(name)[0].mesh.sites), len(M.record(name)[0].mesh.edge_mesh.edges)) for name in CASES}
    assert sizes["C1"] == sizes["C2"] == sizes["C5"] == sizes["C7"] == (1107, 3163) and sizes["C3"] == (516, 1458)
    # C2: every step used ends with dt below the tentative dt -- a psi update failed inside the screening loop, and in
    # steps 1 and 5 not in the first iteration, so that dt shrinks with the loop under way
    _, rec, _ = M.record("C2")
    for k, r in rec.items():
        assert r["whole"]["dt"] < r["before"]["tentative_dt"] and any(a["failed"] for a in r["whole"]["attempts"])
    assert any(a["failed"] for a in rec[0]["single"]["attempts"])
    assert not rec[1]["whole"]["attempts"][0]["failed"] and not rec[5]["whole"]["attempts"][0]["failed"]
    # the others: none fails
    for name in ("C1", "C3", "C5"):
        assert not any(a["failed"] for r in M.record(name)[1].values() for a in r["whole"]["attempts"])
    # C5: dA/dt is at work in every step used (the applied field moved since the step before)
    p, rec, _ = M.record("C5")
    for k, r in rec.items():
        assert np.abs(r["whole"]["A_applied"] - r["before"]["A_applied"]).max() > 1e-6
        assert np.abs(r["whole"]["jn"]).max() > 1.0
    # C7: the failures of a step are spread over several screening iterations, none of which exceeds the budget of
    # max_solve_retries + 1 shrinks while the step as a whole does
    p, rec, _ = M.record("C7")
    budget = p.options.max_solve_retries + 1
    for k, r in rec.items():
        per_iteration, failed = [], 0
        for a in r["whole"]["attempts"]:
            if a["failed"]:
                failed += 1
            else:
                per_iteration.append(failed)
                failed = 0
        assert sum(1 for f in per_iteration if f) >= 2, (k, per_iteration)
        assert max(per_iteration) <= budget < sum(per_iteration), (k, per_iteration)
