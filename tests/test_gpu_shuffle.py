"""The device shuffle (csrc/lgcn_shuffle.hip) started where a test chooses, against numpy itself, bit for bit.

Stream cases: lgcn_np_set_state(key, pos0), then the device shuffle of n -- the grid of tests/shuffle_cases.py, which
tests/test_shuffle_host.py shows to meet every hand-over between k_fy_stream's paths and every rare event of its alignment.
The reference is RandomState.set_state(('MT19937', key, pos0)).shuffle(arange(n)); the generator must go on as numpy's does
(the next shuffle of 700 from the host restatement, not the raw (key, pos): pos = 624 with the old key and pos = 0 with the
twisted one are the same state).

Resolve cases: the swap resolution alone through the test hook lgcn_fy_resolve_device, on J families real draws never give
(one chain of depth n - 1, one run of n - 1 equal targets, shifts around the 256-thread blocks, ramps around the doubling
rounds), against the serial swap loop.

Refusals: a short workspace, n past the device form's limit, n = 0 and n = 1 move neither memory nor the generator."""
import ctypes as C

import numpy as np
import pytest
import torch

import shuffle_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib(pkg):
    lib = pkg._lib.load()
    saved = sc.lib_get_state(lib)
    yield lib
    sc.lib_set_state(lib, *saved)


def _first_diff(got, want):
    bad = np.flatnonzero(got != want)[:5]
    return bad.tolist(), got[bad].tolist(), want[bad].tolist()


@pytest.mark.parametrize("group", sc.GROUPS)
def test_stream_cases(pkg, lib, group):
    U = pkg.utils
    cases = [c for c in sc.stream_cases() if sc.group_of(c[1]) == group]
    assert cases
    for case in cases:
        kid, n, pos0 = case
        want, more = sc.numpy_shuffle(sc.key_of(kid), pos0, n, sc.TAIL)
        sc.lib_set_state(lib, sc.key_of(kid), pos0)
        got = U.shuffle_indices_device(n, DEV).cpu().numpy()
        if not (got.dtype == np.int64 and np.array_equal(got, want)):
            raise AssertionError((case, _first_diff(got, want), sc.ledger_of(case).sequence()))
        cont = U.shuffle_indices(sc.TAIL)
        if not np.array_equal(cont, more):
            raise AssertionError(("generator continues differently", case, _first_diff(cont, more), sc.lib_get_state(lib)[1],
                                  sc.ledger_of(case).final_idx, sc.ledger_of(case).sequence()))


def _resolve(pkg, lib, J, ws=None):
    n = len(J)
    if ws is None:
        ws = torch.empty(int(lib.lgcn_np_shuffle_perm_device_workspace(n)), dtype=torch.uint8, device=DEV)
    perm = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    rc = lib.lgcn_fy_resolve_device(J.ctypes.data, n, pkg._lib.tp(perm), pkg._lib.tp(ws), int(ws.numel()), pkg._lib.current_stream())
    return rc, perm.cpu().numpy()


@pytest.mark.parametrize("n", sc.RESOLVE_NS)
def test_resolve_cases(pkg, lib, n):
    key, pos0 = sc.key_of(1), 333
    _, more = sc.numpy_shuffle(key, pos0, 0, sc.TAIL)
    sc.lib_set_state(lib, key, pos0)
    ws = torch.empty(int(lib.lgcn_np_shuffle_perm_device_workspace(n)), dtype=torch.uint8, device=DEV)
    for name in sc.family_names(n):
        J = sc.family_J(name, n)
        rc, got = _resolve(pkg, lib, J, ws)
        assert rc == 0, (name, n, lib.lgcn_last_error())
        want = sc.resolve_want(name, n)
        assert np.array_equal(got, want), (name, n, _first_diff(got, want), sc.chain_depth(J))
    k2, p2 = sc.lib_get_state(lib)
    assert p2 == pos0 and np.array_equal(k2, key)
    assert np.array_equal(pkg.utils.shuffle_indices(sc.TAIL), more)          # the host generator goes on as before the calls


def test_refusals_move_nothing(pkg, lib):
    U, tp, stream = pkg.utils, pkg._lib.tp, pkg._lib.current_stream()
    key, pos0, n = sc.key_of(0), 600, 5000
    _, more = sc.numpy_shuffle(key, pos0, 0, sc.TAIL)
    need = int(lib.lgcn_np_shuffle_perm_device_workspace(n))
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    perm = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    J = sc.family_J("chain", n)
    dummy = C.c_void_p(256)

    def calls():
        # (what, the call) for both entry points
        yield "short workspace", lambda: lib.lgcn_np_shuffle_perm_device(n, tp(perm), tp(ws), need - 1, stream), 3
        yield "short workspace, hook", lambda: lib.lgcn_fy_resolve_device(J.ctypes.data, n, tp(perm), tp(ws), need - 1, stream), 3
        yield "n too large", lambda: lib.lgcn_np_shuffle_perm_device(0x7ffffff1, dummy, dummy, 1 << 60, stream), 3
        yield "n too large, hook", lambda: lib.lgcn_fy_resolve_device(dummy, 0x7ffffff1, dummy, dummy, 1 << 60, stream), 3
        yield "n = 0", lambda: lib.lgcn_np_shuffle_perm_device(0, None, None, 0, stream), 0
        yield "n = 0, hook", lambda: lib.lgcn_fy_resolve_device(None, 0, None, None, 0, stream), 0
        yield "n = 1", lambda: lib.lgcn_np_shuffle_perm_device(1, tp(perm), None, 0, stream), 0
        yield "n = 1, hook", lambda: lib.lgcn_fy_resolve_device(J.ctypes.data, 1, tp(perm), None, 0, stream), 0

    for what, call, rc in calls():
        perm.fill_(-7)
        sc.lib_set_state(lib, key, pos0)
        assert call() == rc, (what, lib.lgcn_last_error())
        torch.cuda.synchronize()
        k2, p2 = sc.lib_get_state(lib)
        assert p2 == pos0 and np.array_equal(k2, key), what
        assert np.array_equal(U.shuffle_indices(sc.TAIL), more), what
        got = perm.cpu().numpy()
        if what.startswith("n = 1"):
            assert got[0] == 0 and (got[1:] == -7).all(), what
        else:
            assert (got == -7).all(), what
            assert int(ws.count_nonzero()) == 0, what
    # and the workspace of exactly the size asked for is enough, for both
    sc.lib_set_state(lib, key, pos0)
    assert lib.lgcn_np_shuffle_perm_device(n, tp(perm), tp(ws), need, stream) == 0
    assert np.array_equal(perm.cpu().numpy(), sc.numpy_shuffle(key, pos0, n)[0])
    rc, got = _resolve(pkg, lib, J, ws)
    assert rc == 0 and np.array_equal(got, sc.resolve_want("chain", n))
