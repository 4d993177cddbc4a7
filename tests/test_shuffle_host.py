"""The device shuffle (csrc/lgcn_shuffle.hip), what needs no device: the path model of k_fy_stream is pinned to numpy, the
committed stream cases meet every hand-over between the kernel's paths and every rare event (a CONDITION on the case list, so
that tests/test_gpu_shuffle.py is known to run them), deep chains are shown to need the doubling rounds that draws from
MT19937 never need, the host restatement started from a chosen state equals numpy, and the test hook refuses a bad J."""
import ctypes as C
import collections

import numpy as np
import pytest

import shuffle_cases as sc


@pytest.fixture(scope="module")
def lib(pkg):
    lib = pkg._lib.load()
    saved = sc.lib_get_state(lib)
    yield lib
    sc.lib_set_state(lib, *saved)                 # the process-wide generator is left as it was found


def test_model_reproduces_numpy():
    """The model's J, applied by the plain swap loop, is RandomState.shuffle from the same state, and the model stops on the
    word numpy stops on (the next 16 raw words agree), for every stream case."""
    for case in sc.stream_cases():
        kid, n, pos0 = case
        led = sc.ledger_of(case)
        assert led.J[0] == 0 and (led.J <= np.arange(n)).all(), case
        rs = sc.numpy_state(sc.key_of(kid), pos0)
        want = np.arange(n, dtype=np.int64)
        rs.shuffle(want)
        got = sc.swap_loop(led.J)
        assert np.array_equal(got, want), (case, np.flatnonzero(got != want)[:5], led.sequence())
        after = rs.get_state()
        assert np.array_equal(sc.raw_words(after[1], after[2], 16), sc.raw_words(sc.key_of(kid), pos0, led.draws + 16)[-16:]), case
        assert led.final_idx == (after[2] if led.draws else min(pos0, sc.MT_N)), case


def test_ledger_condition():
    """Over the committed cases: no hand-over occurs that the code does not permit, every one it permits occurs, and every
    rare event occurs -- among them the fast guard met with equality and missed by exactly one at each boundary the grid aims at."""
    hand, events = collections.Counter(), collections.Counter()
    for case in sc.stream_cases():
        led = sc.ledger_of(case)
        hand.update(led.handovers)
        events.update(led.events)
    print("hand-overs:", sorted(hand.items(), key=str))
    print("events:", sorted(events.items(), key=str))
    assert set(hand) - sc.HANDOVERS == set()
    assert sc.HANDOVERS - set(hand) == set()
    assert sc.EVENTS - set(events) == set()
    assert len(sc.HANDOVERS) == 26 and len(sc.EVENTS) == 21
    # the one crafted case is what meets fast -> twist -> serial_boundary, and nothing else does
    crafted = sc.ledger_of(("all_accepted", 1649, sc.MT_N))
    assert crafted.handovers[("fast", 1, "serial_boundary")] == hand[("fast", 1, "serial_boundary")] == 1


def test_crafted_key_is_a_numpy_state():
    """key_before_block: numpy itself, set to (key, 624), outputs the chosen words (all but word 0)."""
    rng = np.random.Generator(np.random.PCG64(5))
    words = rng.integers(0, 1 << 32, sc.MT_N)
    key, got = sc.key_before_block(words)
    assert np.array_equal(got[1:], words[1:])
    assert np.array_equal(sc.raw_words(key, sc.MT_N, sc.MT_N), got)
    first = sc.raw_words(sc.key_of("all_accepted"), sc.MT_N, sc.MT_N)
    assert ((first[1:] & 2047) < 1024).all()


def test_resolution_needs_its_rounds_only_on_deep_chains():
    """The numpy form of stage 3 equals the swap loop on every J family at every size.  Capped at 6 of its doubling rounds it
    still does on uniform J (chains about log n deep: at most 14 hops up to n = 100 000 -- what MT19937 draws give), and it
    does not on J[i] = i - 1, one chain of depth n - 1: a device test fed by real draws cannot tell whether the rounds are
    enough, which buffer holds the last round, or how a long run of equal targets is searched."""
    for n in sc.RESOLVE_NS:
        for name in sc.family_names(n):
            J = sc.family_J(name, n)
            want = sc.resolve_want(name, n)
            assert sorted(want.tolist()) == list(range(n)), (name, n)
            got = sc.resolve(J)
            assert np.array_equal(got, want), (name, n, np.flatnonzero(got != want)[:5])
            if name.startswith("uniform"):
                assert sc.chain_depth(J) <= 64 and np.array_equal(sc.resolve(J, max_rounds=6), want), (name, n, sc.chain_depth(J))
    for n in (257, 4097, 65537):
        J = sc.family_J("chain", n)
        assert sc.chain_depth(J) == n - 1 and sc.resolve_rounds(n) > 6
        assert not np.array_equal(sc.resolve(J, max_rounds=6), sc.resolve_want("chain", n)), n
        assert sc.chain_depth(sc.family_J("zero", n)) == 1 and sc.chain_depth(sc.family_J("identity", n)) == 0
    assert [sc.resolve_rounds(n) for n in (2, 3, 4096, 4097, 65536, 65537)] == [1, 2, 12, 13, 16, 17]
    # the sizes that step the sort's bit count: (n + 1)^2 crosses 2^15 and 2^17
    assert 181 ** 2 < 2 ** 15 <= 182 ** 2 and 362 ** 2 < 2 ** 17 <= 363 ** 2


def test_model_J_chains_are_shallow():
    """... and the J of real draws is shallow: the deepest chain over all stream cases."""
    deepest = max(sc.chain_depth(sc.ledger_of(c).J) for c in sc.stream_cases() if c[1] > 60000 and c[2] == 0)
    print("deepest chain of the stream cases with n > 60 000 and pos0 = 0:", deepest)
    assert deepest <= 64


def test_host_restatement_from_a_chosen_state(lib, pkg):
    """lgcn_np_shuffle_perm started from lgcn_np_set_state(key, pos0) equals numpy from the same state, and so does the next
    shuffle on the same stream, for every stream case."""
    U = pkg.utils
    for case in sc.stream_cases():
        kid, n, pos0 = case
        want, more = sc.numpy_shuffle(sc.key_of(kid), pos0, n, sc.TAIL)
        sc.lib_set_state(lib, sc.key_of(kid), pos0)
        got = U.shuffle_indices(n)
        assert np.array_equal(got, want), (case, np.flatnonzero(got != want)[:5])
        assert np.array_equal(U.shuffle_indices(sc.TAIL), more), case


def test_state_round_trip(lib, pkg):
    rng = np.random.Generator(np.random.PCG64(99))
    for pos in (0, 1, 311, 623, 624):
        key = rng.integers(0, 1 << 32, sc.MT_N, dtype=np.uint64).astype(np.uint32)
        sc.lib_set_state(lib, key, pos)
        k2, p2 = sc.lib_get_state(lib)
        assert p2 == pos and np.array_equal(k2, key)
    sc.lib_set_state(lib, key, 1000)              # positions past the block are the block's end
    assert sc.lib_get_state(lib)[1] == sc.MT_N
    # numpy's own state goes in and comes out: seed, draw, hand over, draw on, hand back
    rs = np.random.RandomState(2020)
    rs.randint(0, 1000, size=777)
    st = rs.get_state()
    sc.lib_set_state(lib, st[1], st[2])
    a = np.arange(5000); rs.shuffle(a)
    assert np.array_equal(pkg.utils.shuffle_indices(5000), a)
    k2, p2 = sc.lib_get_state(lib)
    rs2 = sc.numpy_state(k2, p2)
    b = np.arange(3000); rs.shuffle(b)
    c = np.arange(3000); rs2.shuffle(c)
    assert np.array_equal(b, c)


def test_resolve_hook_refuses_bad_targets(lib):
    """J[0] != 0 or J[i] > i: rc 3 before anything is launched (no device is needed to be refused), generator untouched."""
    key = sc.key_of(0)
    sc.lib_set_state(lib, key, 17)
    dummy = C.c_void_p(256)                       # never dereferenced: the refusal comes first
    n = 1000
    good = sc.family_J("half", n)
    for at, value in ((0, 1), (1, 2), (5, 6), (n - 1, n), (n - 1, 0xffffffff), (500, 0x80000000)):
        J = good.copy()
        J[at] = value
        assert lib.lgcn_fy_resolve_device(J.ctypes.data, n, dummy, dummy, 1 << 40, None) == 3, (at, value)
        assert b"fy_resolve_device: J[" in lib.lgcn_last_error()
    assert lib.lgcn_fy_resolve_device(None, n, dummy, dummy, 1 << 40, None) == 3
    assert lib.lgcn_fy_resolve_device(good.ctypes.data, n, None, dummy, 1 << 40, None) == 3
    assert lib.lgcn_fy_resolve_device(good.ctypes.data, -1, dummy, dummy, 1 << 40, None) == 3
    assert lib.lgcn_fy_resolve_device(dummy, 0x7ffffff1, dummy, dummy, 1 << 40, None) == 3      # J is not read either
    assert lib.lgcn_fy_resolve_device(None, 0, None, None, 0, None) == 0
    k2, p2 = sc.lib_get_state(lib)
    assert p2 == 17 and np.array_equal(k2, key)
