"""CPU checks of the cluster-ensemble boundary (gh_ens_*, SPEC §11): every
entry point is exported and bound, the structs have the header's sizes, every
bad argument is refused with GH_EINVAL before a device is looked for (no handle
comes back), and without a gfx950 device gh_ens_create fails with GH_ENODEV:
there is no CPU fallback."""
import ctypes as C

import numpy as np
import pytest

ENTRY_POINTS = ("gh_ens_create", "gh_ens_destroy", "gh_ens_last_error", "gh_ens_init_full", "gh_ens_import_state",
                "gh_ens_export_state", "gh_ens_set_loss", "gh_ens_apply_events", "gh_ens_step", "gh_ens_read_failed",
                "gh_ens_read_detect")


@pytest.fixture(scope="module")
def abi():
    from conftest import PKG_DIR
    from gossipsim import _abi
    if not _abi.LIB_PATH.exists():
        import subprocess
        subprocess.run(["make", "-s", "-C", str(PKG_DIR)], check=True)
    _abi.load()
    return _abi


def params(abi, b, t_fail=5, t_cleanup=5):
    arr = (abi.EnsParams * b)()
    for x in range(b):
        arr[x] = abi.EnsParams(0x5EED0001 + x, t_fail, t_cleanup)
    return arr


def test_symbols_exported_and_bound(abi):
    lib = C.CDLL(str(abi.LIB_PATH))
    bound = {n for n, _, _ in abi.SYMBOLS}
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in bound, name
    assert {n for n in bound if n.startswith("gh_ens_")} == set(ENTRY_POINTS)


def test_struct_sizes(abi):
    assert C.sizeof(abi.EnsConfig) == 32
    assert C.sizeof(abi.EnsParams) == 16
    assert C.sizeof(abi.EnsStats) == 112
    assert len(abi.ENS_STATS) == 14 and abi.ENS_STATS[:10] == tuple(n for n, _ in abi.RoundStats._fields_)
    assert abi.GH_ENS_MAX_MEMBERS == 128


BAD_CONFIGS = {
    "n=1": dict(n=1), "n=0": dict(n=0), "n=-3": dict(n=-3), "n=129": dict(n=129),
    "B=0": dict(b=0), "B=-1": dict(b=-1),
    "k=0": dict(k=0), "k=9": dict(k=9), "k=-1": dict(k=-1),
    "min_members=-1": dict(mm=-1),
}


@pytest.mark.parametrize("kw", BAD_CONFIGS.values(), ids=BAD_CONFIGS.keys())
def test_create_refuses_bad_config(abi, kw):
    lib = abi.load()
    cfg = abi.EnsConfig(kw.get("n", 16), kw.get("b", 2), kw.get("k", 3), kw.get("mm", 4), 0)
    h = C.c_void_p(0x1234)  # (a failed create leaves *h NULL)
    assert lib.gh_ens_create(C.byref(cfg), params(abi, 2), C.byref(h)) == abi.GH_EINVAL
    assert not h.value


@pytest.mark.parametrize("field", ["t_fail", "t_cleanup"])
def test_create_refuses_negative_timeouts(abi, field):
    lib = abi.load()
    cfg = abi.EnsConfig(16, 3, 3, 4, 0)
    par = params(abi, 3)
    setattr(par[2], field, -1)  # (the last cluster's: every entry is checked)
    h = C.c_void_p()
    assert lib.gh_ens_create(C.byref(cfg), par, C.byref(h)) == abi.GH_EINVAL
    assert not h.value


def test_create_refuses_null_pointers(abi):
    lib = abi.load()
    cfg = abi.EnsConfig(16, 2, 3, 4, 0)
    h = C.c_void_p()
    assert lib.gh_ens_create(None, params(abi, 2), C.byref(h)) == abi.GH_EINVAL
    assert not h.value
    assert lib.gh_ens_create(C.byref(cfg), None, C.byref(h)) == abi.GH_EINVAL
    assert not h.value
    assert lib.gh_ens_create(C.byref(cfg), params(abi, 2), None) == abi.GH_EINVAL


def test_null_handle_is_refused_everywhere(abi):
    lib = abi.load()
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data_as(C.c_void_p)
    ev = (abi.Event * 1)(abi.Event(abi.GH_EV_CRASH, 0))
    assert lib.gh_ens_init_full(None, 2, 0, 0) == abi.GH_EINVAL
    assert lib.gh_ens_import_state(None, 0, p, p, p, 0) == abi.GH_EINVAL
    assert lib.gh_ens_export_state(None, 0, 1, p, p, p, p) == abi.GH_EINVAL
    assert lib.gh_ens_set_loss(None, None, None) == abi.GH_EINVAL
    assert lib.gh_ens_apply_events(None, 0, ev, 1) == abi.GH_EINVAL
    assert lib.gh_ens_step(None, 1, None) == abi.GH_EINVAL
    assert lib.gh_ens_read_failed(None, p) == abi.GH_EINVAL
    assert lib.gh_ens_read_detect(None, p, p) == abi.GH_EINVAL
    assert lib.gh_ens_last_error(None) == b"null handle"
    lib.gh_ens_destroy(None)  # a no-op


def test_python_facade_refuses_bad_shapes(abi):
    from gossipsim import Ensemble, GossipError
    for kw in (dict(n=1, clusters=2), dict(n=129, clusters=2), dict(n=16, clusters=0), dict(n=16, clusters=2, fanout=9),
               dict(n=16, clusters=2, min_members=-1), dict(n=16, clusters=2, t_fail=[5, -1])):
        with pytest.raises(GossipError) as ei:
            Ensemble(**kw)
        assert ei.value.code == abi.GH_EINVAL, kw


def test_no_cpu_fallback(abi):
    """Without a gfx950 device gh_ens_create must fail (GH_ENODEV), never emulate."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = abi.load()
    cfg = abi.EnsConfig(16, 2, 3, 4, 0)
    h = C.c_void_p()
    assert lib.gh_ens_create(C.byref(cfg), params(abi, 2), C.byref(h)) == abi.GH_ENODEV
    assert not h.value
    from gossipsim import Ensemble, GossipError
    with pytest.raises(GossipError) as ei:
        Ensemble(16, 2)
    assert ei.value.code == abi.GH_ENODEV
