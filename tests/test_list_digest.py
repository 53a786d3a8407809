"""The recorded listsim runs of tests/list_digest.py are what listsim gives:
the first rounds of every case replayed on the CPU (the whole replay takes a
minute per case, which is why it is recorded)."""
import pytest

import list_digest as ld


@pytest.mark.parametrize("case", sorted(ld.CASES))
def test_recorded_run_is_listsims(case):
    gold = ld.load()[case]
    assert len(gold) == ld.ROUNDS
    got = ld.replay(case, 2)
    assert got == gold[:2]
    assert any(x["dual"] for x in got)  # double entries at introducer 157 from the start
