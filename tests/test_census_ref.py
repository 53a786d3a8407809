"""CPU checks of the census yardstick (tests/census_ref.py) against a plain
double loop over the definitions of include/gossiphip.h (gh_census), and of
the entry point's argument check, which needs no device."""
import ctypes as C

import numpy as np
import pytest

from census_ref import BINS, assert_census_equal, census_ref, CensusRef
from conftest import PKG_DIR

N = 24


def loop_census(hb, ts, alive, R):
    n = len(alive)
    listed, tomb = [0] * n, [0] * n
    lo, hi, am, sm = [-1] * n, [-1] * n, [-1] * n, [0] * n
    hist = [0] * BINS
    for c in range(n):
        for i in range(n):
            if not alive[i] or i == c:
                continue
            x = int(hb[i][c])
            if x == -2:
                tomb[c] += 1
            if x < 0:
                continue
            age = max(0, R + 1 - int(ts[i][c]))
            listed[c] += 1
            lo[c] = x if lo[c] < 0 else min(lo[c], x)
            hi[c] = max(hi[c], x)
            am[c] = max(am[c], age)
            sm[c] += x
            hist[min(age, BINS - 1)] += 1
    i32 = lambda v: np.asarray(v, np.int32)  # noqa: E731
    return CensusRef(i32(listed), i32(tomb), i32(lo), i32(hi), np.asarray(sm, np.int64), i32(am),
                     np.asarray(hist, np.int64))


def random_state(seed, R):
    """Absent cells, tombstones, dead rows, ts in the future, ages past the
    last bin, one column nobody lists and one only its owner lists."""
    rng = np.random.default_rng(seed)
    hb = rng.integers(0, 3000, (N, N))
    kind = rng.random((N, N))
    hb[kind < 0.15] = -1
    hb[(kind >= 0.15) & (kind < 0.3)] = -2
    ts = R + 1 - rng.integers(0, 50, (N, N))  # ages 0..49
    ts[rng.random((N, N)) < 0.1] = R + rng.integers(1, 20)  # ts > R: age 0
    alive = (rng.random(N) < 0.8).astype(np.uint8)
    alive[0] = 1
    hb[:, 5] = -1
    hb[:, 9] = -1
    hb[9, 9] = 77
    return hb.astype(np.int32), ts.astype(np.int32), alive


@pytest.mark.parametrize("seed", range(6))
def test_ref_matches_double_loop(seed):
    R = 40 + 13 * seed
    hb, ts, alive = random_state(seed, R)
    assert (hb == -1).any() and (hb == -2).any() and not alive.all()
    assert (ts > R).any() and (R + 1 - ts.astype(np.int64) > BINS - 1).any()
    ref = census_ref(hb, ts, alive, R)
    assert_census_equal(ref, loop_census(hb, ts, alive, R), f"seed {seed}")
    assert ref.age_hist.sum() == ref.listed.sum()
    for c in (5, 9):  # nobody lists 5; 9 is listed by itself alone, and the diagonal does not count
        assert (ref.listed[c], ref.hb_min[c], ref.hb_max[c], ref.hb_sum[c], ref.age_max[c]) == (0, -1, -1, 0, -1)


def test_ref_skips_dead_rows_and_diagonal():
    hb = np.full((3, 3), 10, np.int32)
    hb[1, 0] = -2
    hb[2, 0] = 7
    ts = np.zeros((3, 3), np.int32)
    ref = census_ref(hb, ts, np.array([1, 1, 0], np.uint8), 4)
    np.testing.assert_array_equal(ref.listed, [0, 1, 2])  # row 2 is stopped: its 7 is not a view
    np.testing.assert_array_equal(ref.tombstoned, [1, 0, 0])
    np.testing.assert_array_equal(ref.age_hist[:6], [0, 0, 0, 0, 0, 3])


def test_census_null_handle_is_einval():
    from gossipsim import _abi
    if not _abi.LIB_PATH.exists():
        import subprocess
        subprocess.run(["make", "-s", "-C", str(PKG_DIR)], check=True)
    lib = _abi.load()
    assert _abi.GH_CENSUS_BINS == BINS
    hist = (C.c_int64 * BINS)()
    assert lib.gh_census(None, None, None, None, None, None, None, hist) == _abi.GH_EINVAL
