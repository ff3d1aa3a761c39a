"""CPU: the scenarios of tests/step_variants.py hit what they claim - checked on the oracle alone, so that the GPU matrix (tests/test_hip_step_variants.py) cannot
pass without exercising the cold instances, the episode ends and the fills it is there for.  Conditions on the inputs, not on the code under test."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import step_variants as V      # noqa: E402


def test_the_rows_span_every_pair_of_levels_and_hold_the_named_ones():
    assert V.uncovered_pairs() == []
    assert 18 <= len(V.ROWS) <= 24 and len(set(V.NAMES)) == len(V.ROWS)
    has = lambda **kw: any(all(r[k] == v for k, v in kw.items()) for r in V.ROWS)      # noqa: E731
    assert has(path="step", book="cold", tape=False, tile=256) and has(path="step", book="cold", tape=False, tile=512)
    assert has(path="step_info", book="cold") and has(path="rollout", book="cold", tile=256) and has(path="run_random", book="spilled")
    for path in ("step", "step_info", "run_random", "rollout_tape"):
        assert has(path=path, tape=True, book="shallow"), path
    assert has(path="step", tape=True, book="cold") and has(path="run_random", tape=True, book="cold")
    for r in V.ROWS:
        assert r["N"] in (38, 41) and 5 <= r["max_step"] <= 7 and r["N"] % 4 != 0 and r["N"] % 16 != 0
        assert r["tape"] == (r["path"] == "rollout_tape") or not r["path"].startswith("rollout")
        if r["path"].startswith("rollout"):
            assert V.n_steps(r) == 4 * V.horizon(r)


@pytest.mark.parametrize("row", V.ROWS, ids=V.NAMES)
def test_the_row_meets_its_claims_on_the_oracle(row):
    """cold / spilled: at least three quarters of the markets start their first episode's last step with n_bids + n_asks + agents > tile (and one of those steps
    fills); shallow: no step of any market starts that way; at least 2 N episodes end; a small-cash row ends an episode `terminated` with a non-zero done mask; a
    last step with a fill; NAV conserved in every episode (the prefill moves cash into cash_on_hold); a prefilled run_random row hands a market that started hot to
    the general build in the middle of its episode.  A rollout row is played here under a stand-in action law - the GPU test checks the same on the policy's actions."""
    run, _ = V.oracle_run(row)
    c = V.claims(row, run.steps)
    print(f"\n[step variants] {V.name_of(row)}: {c}")
    assert (run.ora.flags() == 0).all()
    V.check_claims(row, c, run.em.violating)
    run.close()
