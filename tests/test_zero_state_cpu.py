"""SubgcRecurrence.zero_state (the switch that keeps step 0 of the train decoder from multiplying by the zero initial state) is the LAST
field of the argument block, so every earlier offset keeps its place, and the Python mirror sets it."""
from subgc import _lib, ops


def test_zero_state_is_the_last_field_of_the_argument_block():
    S = _lib.parse_struct("SubgcRecurrence")
    assert S._fields_[-1][0] == "zero_state"
    assert [n for n, _ in S._fields_].count("zero_state") == 1
    assert getattr(S, "zero_state").offset == max(getattr(S, n).offset for n, _ in S._fields_)


def test_recurrence_sets_zero_state():
    assert ops.Recurrence().st.zero_state == 0                    # not given: today's launches
    assert ops.Recurrence(zero_state=1).st.zero_state == 1
    assert ops.Recurrence(zero_state=int(ops.ZERO_STATE_SKIP)).st.zero_state == 1
