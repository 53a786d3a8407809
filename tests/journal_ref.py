"""The yardstick of the detection journal (gh_journal_*): its definition in
include/gossiphip.h, in plain numpy, fed one round at a time.

JournalRef(n, alive0, mode, log_rounds).observe(r, alive, cnt, dmin, listed)
follows the header's three steps per member (transitions, detection, views)
and the round's log entry. It shares no code with the engine.

What feeds it is what the ABI and the CPU oracle expose after a round
(detection_inputs): the failed bitmap gives D_r; where |D_r| == 1 the
detecting rows (read_detectors) are that member's, so cnt = their number and
dmin = the lowest; where |D_r| > 1 only the sum of cnt (the round's
stats.detections) and the union of the detecting rows are known. Such a round
is observed with exact=False: cnt then only marks D_r, `total` is the sum.
The members of such a round are remembered as `inexact`."""
import numpy as np

OFF, DETECT, VIEWS = 0, 1, 3
BINS = 64
MEMBER_FIELDS = ("stop_round", "start_round", "first_round", "first_detector", "first_count", "last_round",
                 "det_rounds", "detectors", "fp_rounds", "forgotten_round", "known_round")
HIST_FIELDS = ("latency_hist", "forget_hist", "known_hist")
FIELDS = MEMBER_FIELDS + HIST_FIELDS
ROUND_DTYPE = np.dtype([("round", np.int32), ("running", np.int32), ("failed", np.int32),
                        ("false_failed", np.int32), ("detections", np.int64), ("false_detections", np.int64),
                        ("stale_views", np.int64), ("missing_views", np.int64)])
# the three per-member fields that need each round's exact cnt / dmin
COUNT_FIELDS = ("first_detector", "first_count", "detectors")

JOIN, LEAVE, CRASH = 1, 2, 3
# the two N = 1,000 scenarios (full_state start at round 0, pull, k = 4)
CLEAN = dict(n=1000, cfg=dict(fanout=4, seed=0x5EED0C02, t_fail=10, t_cleanup=10), rounds=40,
             sched={3: [(CRASH, 321), (CRASH, 999)], 20: [(JOIN, 321)], 26: [(CRASH, 321)]})
STORM = dict(n=1000, cfg=dict(fanout=4, seed=0x5EED0A01, t_fail=6, t_cleanup=6), rounds=24,
             sched={3: [(CRASH, 321), (CRASH, 7)], 5: [(LEAVE, 600)], 14: [(JOIN, 7)]})


class JournalRef:
    def __init__(self, n, alive0, mode=DETECT, log_rounds=0):
        assert mode in (DETECT, VIEWS)
        self.n, self.mode, self.log_rounds = n, mode, log_rounds
        self.prev = np.asarray(alive0).astype(bool).copy()
        for f in MEMBER_FIELDS:
            zero = f in ("first_count", "det_rounds", "detectors", "fp_rounds")
            setattr(self, f, np.full(n, 0 if zero else -1, np.int64 if f == "detectors" else np.int32))
        for f in HIST_FIELDS:
            setattr(self, f, np.zeros(BINS, np.int64))
        self.log = []        # every round's entry (tuples in ROUND_DTYPE's order)
        self.fd_known = []   # ... whether its false_detections is known
        self.inexact = np.zeros(n, bool)  # members detected in some round observed with exact=False
        self.first_rows = {}              # such a member's candidates for first_detector
        self.total_detections = 0

    def observe(self, r, alive, cnt, dmin, listed=None, exact=True, total=None, rows=None):
        """Round r: alive [N] as the round ran, cnt [N] (> 0: member of D_r)
        and dmin [N]; listed [N] with VIEWS. exact=False: cnt only marks D_r,
        total = the round's detections, rows = the rows that detected."""
        a = np.asarray(alive).astype(bool)
        cnt = np.asarray(cnt, np.int64)
        det = cnt > 0
        running = int(a.sum())
        # 1. transitions
        started, stopped = a & ~self.prev, ~a & self.prev
        self.start_round[started] = r
        self.stop_round[started] = -1
        self.stop_round[stopped] = r
        phase = started | stopped
        self.first_round[phase] = self.first_detector[phase] = -1
        self.first_count[phase] = 0
        self.forgotten_round[phase] = self.known_round[phase] = -1
        for c in np.flatnonzero(phase):
            self.first_rows.pop(int(c), None)
        self.prev = a.copy()
        # 2. detection
        self.det_rounds[det] += 1
        self.detectors[det] += cnt[det]
        self.last_round[det] = r
        self.fp_rounds[det & a] += 1
        first = det & (self.first_round < 0)
        self.first_round[first] = r
        self.first_detector[first] = np.asarray(dmin)[first]
        self.first_count[first] = cnt[first]
        lat = first & ~a & (self.stop_round >= 0)
        np.add.at(self.latency_hist, np.minimum(r - self.stop_round[lat], BINS - 1), 1)
        if not exact:
            self.inexact |= det
            for c in np.flatnonzero(first):
                self.first_rows[int(c)] = np.asarray(rows)
        # 3. views
        stale = missing = -1
        if self.mode == VIEWS:
            L = np.asarray(listed, np.int64)
            fg = ~a & (self.forgotten_round < 0) & (L == 0)
            self.forgotten_round[fg] = r
            fg &= self.stop_round >= 0
            np.add.at(self.forget_hist, np.minimum(r - self.stop_round[fg], BINS - 1), 1)
            kn = a & (self.known_round < 0) & (L == running - 1)
            self.known_round[kn] = r
            kn &= self.start_round >= 0
            np.add.at(self.known_hist, np.minimum(r - self.start_round[kn], BINS - 1), 1)
            stale = int(L[~a].sum())
            missing = int((running - 1 - L[a]).sum())
        # the log entry
        detections = int(cnt.sum()) if exact else int(total)
        if exact:
            fd, known = int(cnt[a].sum()), True
        elif not (det & ~a).any():
            fd, known = detections, True   # every member of D_r runs
        elif not (det & a).any():
            fd, known = 0, True            # none does
        else:
            fd, known = -1, False
        self.total_detections += detections
        self.log.append((r, running, int(det.sum()), int((det & a).sum()), detections, fd, stale, missing))
        self.fd_known.append(known)

    def journal(self):
        return {f: getattr(self, f) for f in FIELDS}

    def rounds(self):
        """(the entries gh_journal_rounds returns, which false_detections are known)."""
        k = min(len(self.log), self.log_rounds)
        return (np.array(self.log[len(self.log) - k:], dtype=ROUND_DTYPE),
                np.array(self.fd_known[len(self.log) - k:], bool))


def failed_set(eng):
    """D of the last round from the failed bitmap."""
    return np.flatnonzero(np.unpackbits(eng.read_failed().view(np.uint8), bitorder="little")[: eng.n])


def detection_inputs(eng, stats):
    """observe()'s detection arguments after eng.step(1) returned `stats`
    (a gossipsim Engine / ShardGroup or the CPU oracle): dict(cnt, dmin,
    exact, total, rows)."""
    n = eng.n
    D = failed_set(eng)
    assert stats["failed_members"] == len(D), (stats, D)
    cnt, dmin = np.zeros(n, np.int64), np.full(n, -1, np.int32)
    rows = np.sort(eng.read_detectors()) if len(D) else np.zeros(0, np.int32)
    if len(D) == 1:
        cnt[D[0]], dmin[D[0]] = len(rows), rows[0]
    else:
        cnt[D] = 1
    return dict(cnt=cnt, dmin=dmin, exact=len(D) <= 1, total=stats["detections"], rows=rows)


def drive(eng, sched, rounds, ref, alive_of, listed_of=None, r0=1, per_round=None):
    """Rounds r0 .. r0 + rounds - 1 on eng, one at a time, each fed to ref.
    alive_of(eng) -> alive [N]; listed_of(eng) -> listed [N] of the table after
    the round (VIEWS); per_round(r) runs after each round. Returns the
    per-round stats."""
    out = []
    for r in range(r0, r0 + rounds):
        if sched.get(r):
            eng.apply_events(sched[r])
        st = eng.step(1)
        assert st["last_round"] == r, (r, st)
        inp = detection_inputs(eng, st)
        # det_cnt is the journal's definition of a detection: where it can be
        # seen alone (one member), it is the step's stats.detections
        if inp["exact"]:
            assert int(inp["cnt"].sum()) == st["detections"], (r, st, inp["rows"])
        ref.observe(r, alive_of(eng), listed=listed_of(eng) if ref.mode == VIEWS else None, **inp)
        out.append(st)
        if per_round:
            per_round(r)
    return out


def assert_journal_equal(got, got_rounds, ref, msg=""):
    """got (a Journal: the fields FIELDS) and got_rounds (journal_rounds())
    against a JournalRef, exactly, dtypes included -- except where the ABI does
    not show the truth: first_detector, first_count and detectors need each
    round's per-member cnt / dmin, which a round with |D_r| > 1 does not expose.
    They are compared member-exactly only for the members whose detection
    rounds were all single-member rounds (not ref.inexact); for the others the
    helper checks what is known: sum(detectors) over all members equals the
    sum of the rounds' detections, detectors >= det_rounds, first_count >= 1
    and at most the round's detecting rows, first_detector one of them. Likewise
    a log entry's false_detections is compared where the reference knows it
    (a single-member round, or a D_r wholly running or wholly stopped), and
    bounded by false_failed <= false_detections <= detections otherwise."""
    want = ref.journal()
    ok = ~ref.inexact
    for f in FIELDS:
        a, b = getattr(got, f), want[f]
        assert a.dtype == b.dtype, f"{msg} {f}: dtype {a.dtype} != {b.dtype}"
        if f in COUNT_FIELDS:
            np.testing.assert_array_equal(a[ok], b[ok], err_msg=f"{msg} {f} (exact members)")
        else:
            np.testing.assert_array_equal(a, b, err_msg=f"{msg} {f}")
    assert int(got.detectors.sum()) == ref.total_detections, f"{msg} sum of detectors"
    bad = ref.inexact
    assert (got.detectors[bad] >= got.det_rounds[bad]).all(), f"{msg} detectors < det_rounds"
    for c in np.flatnonzero(bad & (want["first_round"] >= 0)):
        rows = ref.first_rows.get(int(c))
        if rows is None:  # its first detection was a single-member round
            assert (got.first_detector[c], got.first_count[c]) == (want["first_detector"][c], want["first_count"][c])
            continue
        assert 1 <= got.first_count[c] <= len(rows), f"{msg} first_count[{c}] = {got.first_count[c]}"
        assert got.first_detector[c] in rows, f"{msg} first_detector[{c}] = {got.first_detector[c]}"
    wr, known = ref.rounds()
    assert got_rounds.dtype == wr.dtype and len(got_rounds) == len(wr), f"{msg} rounds: {len(got_rounds)} != {len(wr)}"
    for f in ROUND_DTYPE.names:
        if f == "false_detections":
            np.testing.assert_array_equal(got_rounds[f][known], wr[f][known], err_msg=f"{msg} rounds.{f}")
            u = got_rounds[~known]
            assert ((u["false_failed"] <= u[f]) & (u[f] <= u["detections"])).all(), f"{msg} rounds.{f} bounds"
        else:
            np.testing.assert_array_equal(got_rounds[f], wr[f], err_msg=f"{msg} rounds.{f}")
