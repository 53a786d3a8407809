"""The yardstick of gh_census: the census of an exported state in numpy.

census_ref(hb, ts, alive, R) takes what export_state returns ([N][N] hb, ts,
[N] alive) and the tick R of the last completed round, and follows the
definitions of include/gossiphip.h word for word: for member c, S_c = the
rows i != c with alive[i] and hb[i][c] >= 0, T_c = those with hb[i][c] == -2,
age(i, c) = max(0, R + 1 - ts[i][c]). It shares no code with the engine."""
from collections import namedtuple

import numpy as np

BINS = 32
FIELDS = ("listed", "tombstoned", "hb_min", "hb_max", "hb_sum", "age_max", "age_hist")
CensusRef = namedtuple("CensusRef", FIELDS)
_I32_MAX = np.iinfo(np.int32).max


def census_ref(hb, ts, alive, R):
    hb = np.asarray(hb, np.int64)
    ts = np.asarray(ts, np.int64)
    n = hb.shape[1]
    assert hb.shape == ts.shape == (n, n)
    rows = np.asarray(alive).astype(bool)[:, None] & ~np.eye(n, dtype=bool)
    S = rows & (hb >= 0)
    T = rows & (hb == -2)
    age = np.clip(int(R) + 1 - ts, 0, _I32_MAX)
    listed = S.sum(0)
    none = listed == 0
    hb_min = np.where(none, -1, np.where(S, hb, np.iinfo(np.int64).max).min(0, initial=np.iinfo(np.int64).max))
    hb_max = np.where(S, hb, -1).max(0, initial=-1)
    age_max = np.where(S, age, -1).max(0, initial=-1)
    hb_sum = np.where(S, hb, 0).sum(0)
    hist = np.bincount(np.minimum(age[S], BINS - 1), minlength=BINS)
    return CensusRef(listed.astype(np.int32), T.sum(0).astype(np.int32), hb_min.astype(np.int32),
                     hb_max.astype(np.int32), hb_sum.astype(np.int64), age_max.astype(np.int32),
                     hist.astype(np.int64))


def assert_census_equal(got, want, msg=""):
    """Exact equality of all seven outputs, dtypes included."""
    for name in FIELDS:
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype, f"{msg} {name}: dtype {a.dtype} != {b.dtype}"
        np.testing.assert_array_equal(a, b, err_msg=f"{msg} {name}")
