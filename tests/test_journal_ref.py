"""CPU checks of the detection journal's yardstick (tests/journal_ref.py): the
reference driven by the CPU oracle on the two N = 1,000 scenarios the GPU
tests replay, with the facts the oracle shows asserted; and of the library's
side that needs no device: the three exported symbols, their bindings, the
log entry's layout and the NULL-handle refusal."""
import ctypes as C

import numpy as np
import pytest

import journal_ref as jr
import scenarios as sc
from census_ref import census_ref
from conftest import PKG_DIR


def oracle_alive(orc):
    from oracle import oracle as om
    a = np.empty(orc.n, np.uint8)
    assert om.lib().or_export_state(orc.h, None, None, a.ctypes.data_as(C.c_void_p), 0, orc.n) == 0
    return a


def oracle_listed(orc):
    hb, ts, alive = orc.export_state()
    return census_ref(hb, ts, alive, orc.round).listed


def run_oracle(oracle_mod, scen, mode, log_rounds=64):
    n = scen["n"]
    orc = oracle_mod.Oracle(oracle_mod.default_config(n, **scen["cfg"]))
    try:
        orc.import_state(*sc.full_state(n), 0)
        ref = jr.JournalRef(n, oracle_alive(orc), mode, log_rounds)
        stats = jr.drive(orc, scen["sched"], scen["rounds"], ref, oracle_alive, oracle_listed)
    finally:
        orc.close()
    return ref, stats


@pytest.fixture(scope="module")
def clean(oracle_mod):
    return run_oracle(oracle_mod, jr.CLEAN, jr.VIEWS)


@pytest.fixture(scope="module")
def storm(oracle_mod):
    return run_oracle(oracle_mod, jr.STORM, jr.DETECT)


def test_clean_scenario_latency(clean):
    """Two crashes at round 3 are detected at 13, the rejoined 321 crashes
    again at 26 and is detected at 36: three latencies of T_fail = 10, no
    detection of a running member."""
    ref, stats = clean
    log, known = ref.rounds()
    assert known.all()
    det = {int(e["round"]): (int(e["failed"]), int(e["detections"])) for e in log if e["failed"]}
    assert det == {13: (2, 11), 36: (1, 2)}, det
    want = np.zeros(jr.BINS, np.int64)
    want[10] = 3
    np.testing.assert_array_equal(ref.latency_hist, want)
    assert not ref.fp_rounds.any() and not log["false_failed"].any() and not log["false_detections"].any()
    assert (ref.start_round[321], ref.stop_round[321], ref.first_round[321]) == (20, 26, 36)
    assert (ref.stop_round[999], ref.first_round[999], ref.det_rounds[999], ref.last_round[999]) == (3, 13, 1, 13)
    assert ref.det_rounds[321] == 2 and ref.first_count[321] == 2  # the phase of the second crash
    for e, st in zip(log, stats):
        assert e["detections"] == st["detections"] and e["failed"] == st["failed_members"]
    assert log["running"].tolist() == [1000] * 2 + [998] * 17 + [999] * 6 + [998] * 15


def test_clean_scenario_views(clean):
    """Dissemination: a crashed member is forgotten after its detection, the
    rejoined one is known to everybody a few rounds after its join, and the
    members nobody ever doubted are known from the first round."""
    ref, _ = clean
    log, _ = ref.rounds()
    assert ref.forgotten_round[999] > ref.first_round[999] == 13
    # 999 and 321's two stops: detected T_fail rounds after the stop, REMOVE'd from every list the round after
    assert ref.forget_hist.sum() == 3 and ref.forget_hist[11] == 3
    assert (ref.forgotten_round[999], ref.forgotten_round[321]) == (14, 37)
    # the rejoined 321 (round 20) is in every list at round 24; its second stop opens a new phase
    assert ref.known_hist[4] == 1 and ref.known_hist.sum() == 1 and ref.known_round[321] == -1
    assert log["missing_views"][19:24].tolist() == [3, 3, 3, 3, 0]
    others = np.ones(1000, bool)
    others[[321, 999]] = False
    assert (ref.known_round[others] == 1).all() and (ref.forgotten_round[others] == -1).all()
    assert log["missing_views"][0] == 0 and log["stale_views"][0] == 0
    assert log["stale_views"][2] == 2 * 998  # the crash round: every running row still lists both
    assert log["stale_views"][-1] == 0


def test_storm_scenario_classifies(storm):
    """T_fail = 6 at k = 4 from the synthetic start: false-positive storms
    (faithful behaviour that must be reported). Rounds 7-12 detect
    129 / 7 / 59 / 328 / 433 / 43 members, all but two of round 9 running."""
    ref, stats = storm
    log, known = ref.rounds()
    by_round = {int(e["round"]): e for e in log}
    assert [int(by_round[r]["failed"]) for r in range(7, 13)] == [129, 7, 59, 328, 433, 43]
    assert [int(by_round[r]["failed"] - by_round[r]["false_failed"]) for r in range(7, 13)] == [0, 0, 2, 0, 0, 0]
    assert log["false_failed"].sum() > 0 and (log["failed"] - log["false_failed"]).sum() > 0
    assert ref.fp_rounds.sum() == log["false_failed"].sum()
    assert ref.det_rounds.sum() == log["failed"].sum()
    for e, st in zip(log, stats):
        assert e["detections"] == st["detections"], (e, st)
    assert ref.latency_hist.sum() == 2 and ref.latency_hist[6] == 2  # 321 and 7, T_fail after their crash
    assert (ref.first_round[321], ref.det_rounds[321], ref.fp_rounds[321]) == (9, 1, 0)
    # 7 was detected at 9 too; its rejoin at 14 opens a new phase, the totals stay
    assert (ref.start_round[7], ref.stop_round[7], ref.first_round[7], ref.last_round[7], ref.det_rounds[7]) == \
        (14, -1, -1, 9, 1)
    assert (ref.stop_round[600], ref.det_rounds[600]) == (5, 0)  # a leaver is never detected
    assert not known.all() and known[: 8].all()  # round 9 mixes running and stopped members


def test_ref_rules_by_hand():
    """The three steps on a 4-member toy, every branch once."""
    ref = jr.JournalRef(4, [1, 1, 0, 1], jr.VIEWS, log_rounds=2)
    z = np.zeros(4, np.int64)
    ref.observe(1, [1, 1, 0, 1], z, z - 1, listed=[2, 2, 0, 1])
    assert ref.known_round.tolist() == [1, 1, -1, -1] and ref.forgotten_round.tolist() == [-1, -1, 1, -1]
    assert ref.forget_hist.sum() == 0 and ref.known_hist.sum() == 0  # no stop / start seen: no sample
    ref.observe(2, [1, 0, 1, 1], z, z - 1, listed=[2, 3, 0, 2])    # 1 stops, 2 starts
    assert ref.stop_round.tolist() == [-1, 2, -1, -1] and ref.start_round.tolist() == [-1, -1, 2, -1]
    assert ref.known_round.tolist() == [1, -1, -1, 2]
    ref.observe(3, [1, 0, 1, 1], [0, 2, 0, 1], [-1, 0, -1, 2], listed=[2, 0, 2, 2])
    assert ref.first_round.tolist() == [-1, 3, -1, 3] and ref.first_detector.tolist() == [-1, 0, -1, 2]
    assert ref.fp_rounds.tolist() == [0, 0, 0, 1] and ref.latency_hist[1] == 1 and ref.latency_hist.sum() == 1
    assert ref.forgotten_round[1] == 3 and ref.forget_hist[1] == 1 and ref.known_round[2] == 3 and ref.known_hist[1] == 1
    log, known = ref.rounds()
    assert known.all() and log["round"].tolist() == [2, 3]
    assert log[1].tolist() == (3, 3, 2, 1, 3, 1, 0, 0)
    assert log[0].tolist() == (2, 3, 0, 0, 0, 0, 3, 2)


@pytest.fixture(scope="module")
def abi():
    from gossipsim import _abi
    if not _abi.LIB_PATH.exists():
        import subprocess
        subprocess.run(["make", "-s", "-C", str(PKG_DIR)], check=True)
    _abi.load()
    return _abi


def test_journal_symbols_and_bindings(abi):
    lib = C.CDLL(str(abi.LIB_PATH))
    bound = {n: args for n, _, args in abi.SYMBOLS}
    for name, nargs in (("gh_journal_enable", 3), ("gh_journal_read", 15), ("gh_journal_rounds", 5)):
        assert hasattr(lib, name), name
        assert len(bound[name]) == nargs, name
    assert (abi.GH_JOURNAL_OFF, abi.GH_JOURNAL_DETECT, abi.GH_JOURNAL_VIEWS) == (jr.OFF, jr.DETECT, jr.VIEWS)
    assert abi.GH_JOURNAL_BINS == jr.BINS
    assert lib.gh_abi_version() == 8
    import gossipsim
    assert gossipsim.Journal._fields == jr.FIELDS
    assert gossipsim.JOURNAL_ROUND_DTYPE == jr.ROUND_DTYPE
    for name in ("Journal", "GH_JOURNAL_OFF", "GH_JOURNAL_DETECT", "GH_JOURNAL_VIEWS", "GH_JOURNAL_BINS"):
        assert name in gossipsim.__all__


def test_journal_round_layout(abi):
    assert C.sizeof(abi.JournalRound) == 48 == jr.ROUND_DTYPE.itemsize
    assert tuple(n for n, _ in abi.JournalRound._fields_) == jr.ROUND_DTYPE.names
    for n, _ in abi.JournalRound._fields_:
        assert getattr(abi.JournalRound, n).offset == jr.ROUND_DTYPE.fields[n][1], n


def test_journal_null_handle_is_einval(abi):
    lib = abi.load()
    assert lib.gh_journal_enable(None, abi.GH_JOURNAL_DETECT, 8) == abi.GH_EINVAL
    hist = (C.c_int64 * jr.BINS)()
    assert lib.gh_journal_read(None, *([None] * 11), hist, hist, hist) == abi.GH_EINVAL
    out = (abi.JournalRound * 4)()
    tot, k = C.c_int64(), C.c_int64()
    assert lib.gh_journal_rounds(None, out, 4, C.byref(tot), C.byref(k)) == abi.GH_EINVAL
