"""Call sequences across the entry points (tests/sequence_cases.py) played on the device: every step held to ``reference`` at the
allowance its own test module uses, refused steps refused with the message of their rule, every pass called twice for identical
bytes, and at the end the partition in the state a full pass alone leaves.  One test per (profile, committed seed) and per (fixed
sequence, profile); a test stops at its first failing step and names the steps so far."""
import re
import time

import pytest

from tests import sequence_cases as sq

pytestmark = pytest.mark.gpu

ALL = sq.all_sequences()
MESSAGE = {"pin_active": "pinned (clear the pin first)", "pin_left": "still hold the pin", "unevaluated": "has not been evaluated",
           "no_weights": "weights", "nothing_pending": "no asynchronous evaluation pending", "pi_stale": "other root frequencies"}


def _mk(cs, C):
    from hyphy_amd import hip
    return hip.HipPartition(int(cs["D"]), cs["flat_parents"], int(cs["L"]), cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], C)


def _state(part):
    """(Without the schedule report's "[device memory ...]" part: the passes' scratch, the branch cache, the pinned states and the
    asynchronous staging are blocks a partition allocates at first use and keeps.)"""
    from hyphy_amd import hip
    return dict(reduce_form=part.reduce_form(), last_expm_kernel=hip.last_expm_kernel(),
                schedule_info=re.sub(r"\s*\[device memory[^\]]*\]", "", part.schedule_info()),
                repeat_stats=part.repeat_stats(), prune_kernel_name=part.prune_kernel_name())


def _full_passes_alone(cs, C, steps):
    """The state of a fresh partition after the sequence's first two full passes and its last one (behind an evaluation with nothing
    dirty where the sequence's last full pass follows a partial one: a full pass that follows a full pass persists less)."""
    fulls = [s for s in steps if s["kind"] == "evaluate" and sq.label(s).endswith("full")]
    evals = [s for s in steps if s["kind"] == "evaluate"]
    with _mk(cs, C) as part:
        for s in steps:                                   # (the template set the sequence ends under, where it has one)
            if s["kind"] == "set_templates":
                sq.play(part, s)
                break
        for s in [s for s in steps if s["kind"] == "update_templates"][-1:]:
            sq.play(part, s)
        sq.play(part, fulls[0])
        sq.play(part, fulls[1])
        if not sq.label(evals[-2]).endswith("full"):
            sq.play(part, dict(fulls[1], entry="evaluate" if C == 1 else "categories", update=sq.NONE, q_nodes=sq.NONE, M=None))
        sq.play(part, fulls[-1])
        return _state(part)


@pytest.mark.parametrize("profile,which", ALL, ids=[f"{p}-{s}" for p, s in ALL])
def test_sequence(profile, which, monkeypatch):
    from hyphy_amd import hip
    for k, v in sq.environment(profile).items():
        monkeypatch.setenv(k, v)
    t0 = time.perf_counter()
    cs, C, expect = sq.case(profile), sq.classes(profile), sq.expectations(profile)
    steps = sq.sequence(profile, which)
    m = sq.Model(cs, C)
    worst, so_far, n_full, steady = {}, [], 0, None
    with _mk(cs, C) as part:
        for i, step in enumerate(steps):
            so_far.append(f"{i:2d}  {sq.describe(step)}")
            what = f"{profile} {which} step {i} ({sq.label(step)})"
            try:
                if step["kind"] == "refused":
                    try:
                        sq.play(part, step["inner"])
                    except hip.HipError as e:
                        assert MESSAGE[step["why"]] in str(e), f"refused for another reason: {e}"
                    else:
                        raise AssertionError("the library let the step through")
                    sq.apply(m, step)
                    continue
                got = sq.play(part, step)
                ref = sq.expected(m, step)
                if ref is not None:
                    x = sq.hold_step(what, m, step, got, ref)
                    worst[sq.label(step)] = max(worst.get(sq.label(step), 0.0), x)
            except (AssertionError, hip.HipError) as e:
                raise AssertionError(f"{profile} {which}: step {i} ({sq.describe(step)}): {e}\nthe steps so far:\n" + "\n".join(so_far)) from e
            if sq.label(step).endswith("full"):
                n_full += 1
                if n_full == 2 and expect.get("rerooted"):
                    assert "re-rooted" in part.schedule_info(), part.schedule_info()
                if n_full == 3 and expect.get("in_use"):
                    steady = (part.repeat_stats()["in_use"], part.prune_kernel_name())
        after = _state(part)
    if expect.get("in_use"):
        assert after["repeat_stats"]["in_use"] == 1, after["repeat_stats"]
    if steady is not None and which == "compressed_pass_then_partial":
        assert steady == (1, after["prune_kernel_name"]), (steady, after["prune_kernel_name"])
    alone = _full_passes_alone(cs, C, steps)
    assert after == alone, f"{profile} {which}: the state after the sequence\n{after}\nis not what full passes alone leave\n{alone}"
    print(f"{profile} {which}: {len(steps)} steps in {time.perf_counter() - t0:.2f} s; largest deviation / allowance per entry point: "
          + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))
