"""The stop / keep-best rule of stage "NSFP, v1" as stated on the host (himo_amd/nsfp.py ``stop_rule``): hand-written loss sequences."""
import math


def _rule(losses, patience, min_delta):
    from himo_amd.nsfp import stop_rule
    return stop_rule(losses, patience, min_delta)


def test_strictly_falling_sequence_never_stops_and_keeps_the_last():
    assert _rule([5.0, 4.0, 3.0, 2.0, 1.0], 2, 1e-4) == (5, 0)


def test_plateau_reaching_patience_stops_there_and_later_losses_change_nothing():
    # improves at 1 and 2; 3, 4, 5 are stale: stale reaches patience 3 at iteration 5; the better losses after it are never seen
    assert _rule([3.0, 2.0, 2.0, 2.0, 2.0, 0.5, 0.1], 3, 1e-4) == (2, 5)
    # one short of patience, then an improvement resets the count
    assert _rule([3.0, 2.0, 2.0, 2.0, 1.0, 1.0, 1.0], 3, 1e-4) == (5, 0)
    assert _rule([3.0, 2.0, 2.0, 2.0, 1.0, 1.0, 1.0, 1.0], 3, 1e-4) == (5, 8)


def test_improvement_of_exactly_min_delta_is_not_an_improvement():
    # 1.0 - 0.25 == 0.75 exactly in float64: 0.75 < 0.75 is false; anything below is an improvement
    assert _rule([1.0, 0.75, 0.75], 2, 0.25) == (1, 3)
    assert _rule([1.0, math.nextafter(0.75, 0.0), 0.75], 2, 0.25) == (2, 0)


def test_nan_never_improves_but_counts_as_stale():
    nan = float("nan")
    assert _rule([2.0, nan, 1.0, nan, nan], 2, 0.0) == (3, 5)
    assert _rule([nan, nan, nan], 5, 0.0) == (0, 0)
    assert _rule([nan, nan, nan], 3, 0.0) == (0, 3)


def test_patience_zero_never_stops_but_keeps_the_best():
    assert _rule([2.0, 1.0, 1.5, 1.5, 1.5, 1.5, 0.5, 0.9], 0, 1e-4) == (7, 0)
    assert _rule([2.0, 1.0, 1.5, 1.5], -1, 1e-4) == (2, 0)


def test_empty_sequence():
    assert _rule([], 3, 1e-4) == (0, 0)


def test_huge_min_delta_accepts_only_the_first_loss():
    # +inf - 1e9 is +inf: the first finite loss improves, nothing after it can
    assert _rule([4.0, 3.0, 2.0, 1.0, 0.5, 0.1], 3, 1e9) == (1, 4)
